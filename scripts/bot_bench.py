"""Time mas_bot_act beside mas_policy_act_sel on the same mask and buffer (HIP
events, one process, the calls alternating): 2v2 x 65536 envs, half the agents
selected (mask 0b1100), rows taken from the env after --settle steps the bots
drive.  Each figure is the median of --launches single launches after a
warm-up; --rounds rounds give the spread of repeated medians.  Then a 20-step
self-play rollout (PPOTrainer.rollout_step) with a bot opponent against the
same rollout with a policy opponent, alternating, --rollouts times each.
usage: bot_bench.py [--parent libmas_parent.so] [--envs N] [--rounds R] [--launches L] [--rollouts K]
--parent: also time act_sel of another build of the library (the parent
commit's) in the same process."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gym-ma-survival-2d_amd'))
import torch  # noqa: E402

from masurvival import abi, ppo  # noqa: E402
from masurvival.bots import bot_act  # noqa: E402
from masurvival.config import C3_CONFIG  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

MASK = 0b1100
HORIZON = 20


def median_us(forms, rounds, launches):
    for f in forms.values():
        for i in range(5):
            f(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    med = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            for i, (e0, e1) in enumerate(ev):
                e0.record()
                f(i)
                e1.record()
            torch.cuda.synchronize()
            med[k].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    return med


def calls(args):
    N = args.envs
    env = VecMaSurvival(C3_CONFIG, n_envs=N, seeds=range(N), auto_reset=True)
    A, D, dev = env.n_agents, env.obs_dim, env.device
    cs = env.rc.to_struct()
    M = N * A
    torch.manual_seed(0)
    fp = ppo.FusedPolicy(ppo.PolicyMLP(D).to(dev), D, dev)
    fp.pack()
    xb = fp.x_buffer(M)
    xb[:, :D].copy_(env.reset().reshape(M, D))
    a = torch.zeros((N, A, 6), dtype=torch.int8, device=dev)
    a2 = a.view(-1, 6)
    lp, v = torch.empty((M,), device=dev), torch.empty((M,), device=dev)
    r, d = torch.empty((N, A), device=dev), torch.empty((N,), dtype=torch.uint8, device=dev)
    for _ in range(args.settle):  # rows of a game in progress: agents have met, some are dead
        bot_act(cs, 'hunter', xb, A, 0b0011, a2)
        bot_act(cs, 'forager', xb, A, MASK, a2)
        env.step_x(a, xb, r, d)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    forms = {
        'act_sel': lambda i: fp.act_sel(xb, A, MASK, 1, i, a2, lp, v),
        'bot_hunter': lambda i: bot_act(cs, 'hunter', xb, A, MASK, a2),
        'bot_forager': lambda i: bot_act(cs, 'forager', xb, A, MASK, a2),
        'bot_idle': lambda i: bot_act(cs, 'idle', xb, A, MASK, a2),
    }
    if args.parent:
        plib = ctypes.CDLL(os.path.abspath(args.parent))
        plib.mas_policy_act_sel.restype, plib.mas_policy_act_sel.argtypes = abi.SIGNATURES['mas_policy_act_sel']
        forms = {'parent_act_sel': lambda i: abi.check(plib.mas_policy_act_sel(
            ptr(fp.packed), D, N, A, MASK, 0, ptr(xb), fp.Dx, 1, i, 0, ptr(a2), ptr(lp), ptr(v), None,
            fp._stream())), **forms}
    med = median_us(forms, args.rounds, args.launches)
    env.close()
    for k, ms in med.items():
        print(f'{k:16s} medians [us]: ' + ' '.join(f'{m:7.1f}' for m in ms)
              + f'   min {min(ms):.1f} max {max(ms):.1f}', flush=True)
    return med


def rollouts(args):
    N = args.envs

    def trainer(opponent):
        env = VecMaSurvival(C3_CONFIG, n_envs=N, seeds=range(N), auto_reset=True)
        return ppo.PPOTrainer(env, ppo.PPOConfig(horizon=HORIZON), seed=0, opponent=opponent, learner_agents=[0, 1])
    torch.manual_seed(1)
    probe = VecMaSurvival(C3_CONFIG, n_envs=1, seeds=[0])
    D = probe.obs_dim
    probe.close()
    trs = {'policy_opponent': trainer(ppo.PolicyMLP(D, 256)), 'bot_opponent': trainer('bot:hunter')}
    ms = {k: [] for k in trs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.rollouts + 1):  # the first pass of each is the warm-up
        for k, tr in trs.items():
            e0.record()
            for t in range(HORIZON):
                tr.rollout_step(t)
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:
                ms[k].append(e0.elapsed_time(e1))
            tr.buf.xb[0].copy_(tr.buf.xb[HORIZON])  # the next rollout goes on from the last rows
    for k, v in ms.items():
        print(f'{k:16s} {HORIZON}-step rollout [ms]: ' + ' '.join(f'{m:7.3f}' for m in v)
              + f'   median {statistics.median(v):.3f}', flush=True)
    for tr in trs.values():
        tr.env.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--settle', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=25)
    ap.add_argument('--rollouts', type=int, default=7)
    args = ap.parse_args()
    med = calls(args)
    ms = rollouts(args)
    print(json.dumps({'envs': args.envs, 'mask': MASK, 'launches': args.launches, 'call_median_us': med,
                      'rollout_ms': ms}))


if __name__ == '__main__':
    main()
