"""Time mas_rows_select at the self-play trainer's own shape (2v2 x 65536 envs,
T = 20, D = 160: x rows of 176 bf16) and one iteration() of the self-play
trainer beside the plain trainer (HIP events, one process, the forms
alternating).

select: the five arrays the trainer compacts (x, actions, logp, rewards over
T row blocks, values over T + 1), masks 0b0011 and 0b1111, as
  kernel        the trainer's two mas_rows_select launches
  torch_rows    torch.index_select(dim 0) of each array by the output rows' index
  torch_agents  torch.index_select(dim 1) of each array's [envs, agents, ..] view
the torch forms write into preallocated outputs (out=).  Each figure is the
median of --launches single gathers after a warm-up, once per round; GB/s
counts every byte read and written once.
iteration: rollout / gae (finish_rollout: bootstrap, select, GAE, normalise)
/ update of a plain PPOTrainer and of a self-play one (learner [0, 1], a
frozen opponent) on twin envs.
usage: rows_select_bench.py [--part select|iteration|all] [--rounds R] [--launches L] [--envs N] [--horizon T]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gym-ma-survival-2d_amd'))
import torch  # noqa: E402

from masurvival import ppo  # noqa: E402
from masurvival.config import NAMED_CONFIGS  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402


def ev():
    return torch.cuda.Event(enable_timing=True)


def select_part(args):
    T, N, A, D = args.horizon, args.envs, 4, 160
    Dx = 16 * ((D + 1 + 15) // 16)
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    R, R1 = T * N * A, (T + 1) * N * A
    x = torch.randn((R, Dx), device=dev, generator=g).to(torch.bfloat16)
    act = torch.randint(0, 2, (R, 6), device=dev, generator=g, dtype=torch.int8)
    logp, rew = torch.randn((R,), device=dev, generator=g), torch.randn((R,), device=dev, generator=g)
    val = torch.randn((R1,), device=dev, generator=g)
    out = {}
    for mask in (0b0011, 0b1111):
        agents = [a for a in range(A) if (mask >> a) & 1]
        m = len(agents)
        n, n1 = T * N * m, (T + 1) * N * m
        o = dict(x=torch.empty((n, Dx), dtype=torch.bfloat16, device=dev),
                 act=torch.empty((n, 6), dtype=torch.int8, device=dev), logp=torch.empty((n,), device=dev),
                 rew=torch.empty((n,), device=dev), val=torch.empty((n1,), device=dev))
        ag = torch.tensor(agents, device=dev)
        ridx = (torch.arange(T * N, device=dev).unsqueeze(1) * A + ag).reshape(-1)
        ridx1 = (torch.arange((T + 1) * N, device=dev).unsqueeze(1) * A + ag).reshape(-1)

        def kernel():
            ppo.rows_select(A, mask, x=x, x_out=o['x'], actions=act, actions_out=o['act'],
                            f32=[(logp, o['logp']), (rew, o['rew'])])
            ppo.rows_select(A, mask, f32=[(val, o['val'])])

        def torch_rows():
            torch.index_select(x, 0, ridx, out=o['x'])
            torch.index_select(act, 0, ridx, out=o['act'])
            torch.index_select(logp, 0, ridx, out=o['logp'])
            torch.index_select(rew, 0, ridx, out=o['rew'])
            torch.index_select(val, 0, ridx1, out=o['val'])

        def torch_agents():
            torch.index_select(x.view(-1, A, Dx), 1, ag, out=o['x'].view(-1, m, Dx))
            torch.index_select(act.view(-1, A, 6), 1, ag, out=o['act'].view(-1, m, 6))
            torch.index_select(logp.view(-1, A), 1, ag, out=o['logp'].view(-1, m))
            torch.index_select(rew.view(-1, A), 1, ag, out=o['rew'].view(-1, m))
            torch.index_select(val.view(-1, A), 1, ag, out=o['val'].view(-1, m))

        forms = {'kernel': kernel, 'torch_rows': torch_rows, 'torch_agents': torch_agents}
        # same results (bit for bit) before anything is timed
        ref = None
        for k, f in forms.items():
            for t in o.values():
                t.view(torch.uint8).zero_()
            f()
            torch.cuda.synchronize()
            got = [t.clone().view(torch.uint8) for t in o.values()]
            if ref is None:
                ref = got
            assert all(torch.equal(a, b) for a, b in zip(ref, got)), k
        for f in forms.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        nbytes = 2 * (n * (Dx * 2 + 6 + 4 + 4) + n1 * 4)
        evs = [(ev(), ev()) for _ in range(args.launches)]
        med = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                for e0, e1 in evs:
                    e0.record()
                    f()
                    e1.record()
                torch.cuda.synchronize()
                med[k].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs))
        for k, us in med.items():
            print(f'mask {mask:#06b} {k:13s} medians [us]: ' + ' '.join(f'{u:8.1f}' for u in us)
                  + f'   min {min(us):.1f} max {max(us):.1f}   {nbytes / min(us) * 1e-3:7.1f} GB/s at the min '
                  f'({nbytes / 1e9:.3f} GB read + written)', flush=True)
        out[f'{mask:#06b}'] = {'bytes': nbytes, 'median_us': med}
        del o
    print(json.dumps({'part': 'select', 'T': T, 'envs': N, 'agents': A, 'x_stride': Dx, 'launches': args.launches,
                      'masks': out}), flush=True)


def iteration_part(args):
    T, N = args.horizon, args.envs
    cfg = ppo.PPOConfig(horizon=T)
    envs = [VecMaSurvival(NAMED_CONFIGS['2v2'], n_envs=N, seeds=range(N), auto_reset=True) for _ in range(2)]
    torch.manual_seed(1)
    opp = ppo.PolicyMLP(envs[0].obs_dim, 256)
    trs = {'plain': ppo.PPOTrainer(envs[0], cfg, seed=0),
           'selfplay': ppo.PPOTrainer(envs[1], cfg, seed=0, opponent=opp, learner_agents=[0, 1])}
    res = {k: [] for k in trs}
    for it in range(args.rounds + 1):  # the first round warms up
        for k, tr in trs.items():
            e = [ev() for _ in range(4)]
            e[0].record()
            for t in range(T):
                tr.rollout_step(t)
            e[1].record()
            tr.finish_rollout()
            e[2].record()
            tr.update()
            e[3].record()
            torch.cuda.synchronize()
            ms = [e[i].elapsed_time(e[i + 1]) for i in range(3)]
            if it > 0:
                res[k].append(ms)
            print(f'{"warm-up" if it == 0 else "round %d" % it} {k:9s} rollout {ms[0]:8.2f} ms  gae {ms[1]:7.2f} ms  '
                  f'update {ms[2]:8.2f} ms', flush=True)
    print(json.dumps({'part': 'iteration', 'T': T, 'envs': N, 'minibatches': cfg.minibatches,
                      'ms_rollout_gae_update': res}), flush=True)
    for e_ in envs:
        e_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['select', 'iteration', 'all'], default='all')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--launches', type=int, default=15)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--horizon', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rows_select_bench: needs a GPU (a timing on the CPU says nothing)')
    if args.part in ('select', 'all'):
        select_part(args)
    if args.part in ('iteration', 'all'):
        iteration_part(args)


if __name__ == '__main__':
    main()
