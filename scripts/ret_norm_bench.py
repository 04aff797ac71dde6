"""Kernel times of the reward normalisation at the bench's rollout shape (T=64,
65536 envs x 4 agents): mas_gae, mas_gae_scaled and mas_ret_stats alternating
in one process, one HIP event pair per call; median and min-max per kernel.
MAS_GAE_SCAN=1 in the environment times the scan form of the two GAE calls.
--iteration: PPOTrainer.iteration() of the 2v2 bench shape with reward_norm off
and on instead, two trainers alternating in one process."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gym-ma-survival-2d_amd'))
import torch  # noqa: E402

from masurvival.ppo import gae, gae_scaled, gae_scratch, ret_stats  # noqa: E402

T, N, A = 64, 65536, 4


def iteration_times(rounds=6, per_figure=3, warmup=2):
    from masurvival.ppo import PPOConfig, PPOTrainer
    from masurvival.vec_env import VecMaSurvival
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    with open(os.path.join(root, 'configs', '2v2.json')) as f:
        cfg = json.load(f)
    trs = {}
    for flag in (False, True):
        env = VecMaSurvival(cfg, n_envs=N, seeds=range(N), auto_reset=True)
        trs[flag] = PPOTrainer(env, PPOConfig(horizon=T, reward_norm=flag), seed=0)
        for _ in range(warmup):
            trs[flag].iteration()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for k in range(rounds):
        for flag in (False, True):
            t0 = time.perf_counter()
            for _ in range(per_figure):
                trs[flag].iteration()
            torch.cuda.synchronize()
            ms[flag].append((time.perf_counter() - t0) * 1e3 / per_figure)
        print(f'round {k} off {ms[False][-1]:.3f} ms  on {ms[True][-1]:.3f} ms')
    for flag in (False, True):
        x = ms[flag]
        print(f'reward_norm {flag} ms/iteration: min {min(x):.3f} median {statistics.median(x):.3f} max {max(x):.3f}')
    rn = trs[True].ret_norm
    print(f'reward scale {float(rn.scale[0]):.6g} count {float(rn.count):.0f}')


def kernel_times():
    WARMUP, CALLS = 5, 30
    g = torch.Generator(device='cuda').manual_seed(0)
    r = torch.randn((T, N, A), device='cuda', generator=g)
    v = torch.randn((T + 1, N, A), device='cuda', generator=g)
    d = (torch.rand((T, N), device='cuda', generator=g) < 0.05).to(torch.uint8)
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    sums = torch.empty(2, device='cuda', dtype=torch.float64)
    rsums = torch.empty(2, device='cuda', dtype=torch.float64)
    carry = torch.zeros((N * A,), device='cuda')
    scale = torch.tensor([0.37], device='cuda')
    sc = gae_scratch(N * A, 'cuda')

    gae_bytes = (3 * T + 1) * N * A * 4 + T * N          # rewards, values (T + 1 rows), adv, ret; dones
    ret_bytes = T * N * A * 4 + T * N + 2 * N * A * 4    # rewards, dones; the carry in and out
    calls = {
        'mas_gae': (lambda: gae(r, v, d, 0.99, 0.95, adv, ret, sums, A, scratch=sc), gae_bytes),
        'mas_gae_scaled': (lambda: gae_scaled(r, v, d, 0.99, 0.95, scale, 10.0, adv, ret, sums, A, scratch=sc),
                           gae_bytes + 4),
        'mas_ret_stats': (lambda: ret_stats(r, d, 0.99, carry, rsums, A, scratch=sc), ret_bytes),
    }
    times = {k: [] for k in calls}
    for i in range(WARMUP + CALLS):
        for name, (fn, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= WARMUP:
                times[name].append(e0.elapsed_time(e1) * 1000)
    form = 'scan' if os.environ.get('MAS_GAE_SCAN', '0')[:1] == '1' else 'walk'
    print(f'T={T} N={N} A={A}, {CALLS} timed calls each after {WARMUP} warm-up rounds, alternating; GAE form: {form}')
    for name, (_, nbytes) in calls.items():
        ts = times[name]
        med = statistics.median(ts)
        print(f'{name}: median {med:.1f} us (min {min(ts):.1f}, max {max(ts):.1f}), '
              f'{nbytes / med / 1e6:.2f} TB/s over {nbytes / 1e6:.0f} MB')
    lo, hi = min(times['mas_gae']), max(times['mas_gae'])
    med = statistics.median(times['mas_gae_scaled'])
    print(f'mas_gae_scaled median {med:.1f} us {"within" if lo <= med <= hi else "OUTSIDE"} '
          f"mas_gae's min-max [{lo:.1f}, {hi:.1f}] us")


if __name__ == '__main__':
    iteration_times() if '--iteration' in sys.argv[1:] else kernel_times()
