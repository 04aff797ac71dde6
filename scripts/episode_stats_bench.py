"""Kernel time of the episode statistics at the bench's rollout shape (T=64,
65536 envs x 4 agents, dones at about 0.2 %): mas_ret_stats (the yardstick: it
reads the same rewards and dones) and mas_episode_stats alternating in one
process, one HIP event pair per call; median and min-max per kernel and the
ratio of the medians.  MAS_LIB in the environment times another build of the
library (csrc/Makefile VARIANT=... VFLAGS="-DMAS_EP_WG=... -DMAS_EP_CHUNK=...")."""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gym-ma-survival-2d_amd'))
import torch  # noqa: E402

from masurvival import abi  # noqa: E402
from masurvival.ppo import episode_stats, gae_scratch, ret_stats  # noqa: E402

T, N, A = 64, 65536, 4
P_DONE = 0.002
WARMUP, CALLS = 5, 30


def main():
    g = torch.Generator(device='cuda').manual_seed(0)
    r = torch.randn((T, N, A), device='cuda', generator=g)
    d = (torch.rand((T, N), device='cuda', generator=g) < P_DONE).to(torch.uint8)
    rsums = torch.empty(2, device='cuda', dtype=torch.float64)
    carry = torch.zeros((N * A,), device='cuda')
    sc = gae_scratch(N * A, 'cuda')
    G = torch.zeros((N * A,), device='cuda', dtype=torch.float64)
    ln = torch.zeros((N,), device='cuda', dtype=torch.int32)
    rec = torch.empty(6 + 2 * A, device='cuda', dtype=torch.float64)
    n_scr = abi.load_library().mas_episode_stats_scratch_doubles(N, A)
    esc = torch.empty(n_scr, device='cuda', dtype=torch.float64)

    rollout = T * N * A * 4 + T * N
    calls = {
        'mas_ret_stats': (lambda: ret_stats(r, d, 0.99, carry, rsums, A, scratch=sc), rollout + 2 * N * A * 4),
        'mas_episode_stats': (lambda: episode_stats(r, d, A, G, ln, rec, side_mask=0b0011, scratch=esc),
                              rollout + 2 * N * (A * 8 + 4)),
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
    print(f'library {os.path.basename(abi.LIB_PATH)}: T={T} N={N} A={A}, dones {float(d.float().mean()) * 100:.2f} %, '
          f'{CALLS} timed calls each after {WARMUP} warm-up rounds, alternating; '
          f'{n_scr // (6 + 2 * A)} workgroups of {(N * (6 + 2 * A) + n_scr - 1) // n_scr} envs')
    for name, (_, nbytes) in calls.items():
        ts = times[name]
        med = statistics.median(ts)
        print(f'{name}: median {med:.1f} us (min {min(ts):.1f}, max {max(ts):.1f}), '
              f'{nbytes / med / 1e6:.2f} TB/s over {nbytes / 1e6:.1f} MB')
    lo, hi = min(times['mas_ret_stats']), max(times['mas_ret_stats'])
    med, ref = statistics.median(times['mas_episode_stats']), statistics.median(times['mas_ret_stats'])
    print(f'mas_episode_stats / mas_ret_stats medians: {med / ref:.2f}; mas_episode_stats median '
          f'{"within" if lo <= med <= hi else "OUTSIDE"} mas_ret_stats\' min-max [{lo:.1f}, {hi:.1f}] us')
    print(f'record of the last call: {rec.tolist()}')


if __name__ == '__main__':
    main()
