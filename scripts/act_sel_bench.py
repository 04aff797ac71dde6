"""Time mas_policy_act_sel against mas_policy_act_x (HIP events, one process,
the kernels alternating): 262144 rows (65536 envs x 4 agents), D = 160.  Each
figure is the median of --launches single launches after a warm-up; --rounds
rounds give act_x's own spread over repeated medians to compare against.
usage: act_sel_bench.py [--parent libmas_parent.so] [--rounds R] [--launches L]
--parent: also time act_x of another build of the library (the parent commit's)
in the same process."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=25)
    args = ap.parse_args()
    D, N, A = 160, 65536, 4
    M = N * A
    dev = torch.device('cuda')
    torch.manual_seed(0)
    fp = ppo.FusedPolicy(ppo.PolicyMLP(D).to(dev), D, dev)
    fp.pack()
    xb = fp.x_buffer(M)
    xb[:, :D] = (torch.randn((M, D), device=dev) * 3.0).to(torch.bfloat16)
    a = torch.empty((M, 6), dtype=torch.int8, device=dev)
    lp = torch.empty((M,), device=dev)
    v = torch.empty((M,), device=dev)
    lg = torch.empty((M, 16), device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    forms = {
        'act_x': lambda i: fp.act_x(xb, 1, i, a, lp, v),
        'sel_full': lambda i: fp.act_sel(xb, A, 0b1111, 1, i, a, lp, v),
        'sel_half': lambda i: fp.act_sel(xb, A, 0b0011, 1, i, a, lp, v),
        'sel_full_greedy': lambda i: fp.act_sel(xb, A, 0b1111, 1, i, a, lp, v, greedy=True),
        'sel_full_logits': lambda i: fp.act_sel(xb, A, 0b1111, 1, i, a, lp, v, logits=lg),
    }
    if args.parent:
        plib = ctypes.CDLL(os.path.abspath(args.parent))
        plib.mas_policy_act_x.restype, plib.mas_policy_act_x.argtypes = abi.SIGNATURES['mas_policy_act_x']
        forms = {'parent_act_x': lambda i: abi.check(plib.mas_policy_act_x(
            ptr(fp.packed), D, M, 0, ptr(xb), fp.Dx, 1, i, ptr(a), ptr(lp), ptr(v), fp._stream())), **forms}
    for f in forms.values():
        for i in range(5):
            f(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    med = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            for i, (e0, e1) in enumerate(ev):
                e0.record()
                f(i)
                e1.record()
            torch.cuda.synchronize()
            med[k].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    for k, ms in med.items():
        print(f'{k:16s} medians [us]: ' + ' '.join(f'{m:7.1f}' for m in ms)
              + f'   min {min(ms):.1f} max {max(ms):.1f}', flush=True)
    print(json.dumps({'rows': M, 'obs_dim': D, 'launches': args.launches, 'median_us': med}))


if __name__ == '__main__':
    main()
