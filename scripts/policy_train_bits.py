"""Compare what the PPO train kernels of two libraries store, byte for byte:
every (path, D, M, policy kind, coefficient set) case of
tests/test_gpu_policy_rows.py (its CASES, PATHS, input builders and
sentinel-filled Buffers, imported, not restated) through mas_policy_train_ld /
mas_policy_train_rm, plus two mas_policy_train_dw3 calls (D = 160, M = 512 and
D = 138, M = 256).  Each case's inputs are built once (the batch from the first
library's stored h2, as the test builds it) and given to every library; the
whole of h1, h2, dz, dA2, dA1 and the partials -- padding and sentinel rows
included -- and the dw3_out of the DW3 calls are compared with the first
library's.  One line per case; exit status 1 on any difference.
usage: policy_train_bits.py libA.so libB.so [...]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ('tests', 'gym-ma-survival-2d_amd'):
    sys.path.insert(0, os.path.join(ROOT, d))
import pytest  # noqa: E402
import torch  # noqa: E402

import policy_rows_ref as R  # noqa: E402
import test_gpu_policy_rows as T  # noqa: E402
from masurvival import abi, ppo  # noqa: E402

DW3_CASES = [(160, 512), (138, 256)]


def load(path):
    abi._lib = None
    return abi.load_library(path)


def raw(t):
    return t.contiguous().view(torch.uint8).flatten().cpu()


def train_outputs(lib, mp, path, D, M, kind, cset, inputs):
    """The buffers of one mas_policy_train_ld / _rm call as bytes; inputs
    (xb, batch) None: built here from this library's stored h2."""
    ppo.load_library = lambda: lib
    rm = path == 'rm'
    T._setenv(mp, path)
    p, fp = T._policy(D, kind, rm, mp)
    cf = R.coef(cset, M)
    B = T.Buffers(lib, M, rm)
    if inputs is None:
        xb, g = T._rows(fp, D, M)
        null = (torch.zeros((M, 6), dtype=torch.int8, device='cuda'),) + tuple(torch.zeros(M, device='cuda')
                                                                                for _ in range(3))
        B.run(fp, xb, null, cf)
        inputs = (xb, R.make_batch(R.params(p), xb[:, :D], cf, g, h2=B.outputs(fp)['h2']))
        B.refill()
    B.run(fp, *inputs, cf)
    out = {k: raw(v) for k, v in B.t.items()}
    out['partials'] = raw(B.part)
    return out, inputs


def dw3_outputs(lib, mp, D, M, inputs):
    """The same for one mas_policy_train_dw3 call (h2 and dz stay sentinels), with its dw3_out."""
    ppo.load_library = lambda: lib
    T._setenv(mp, 'db')
    mp.delenv('MAS_POL_DW3', raising=False)
    p, fp = T._policy(D, 'plain')
    clip, vf, ec, sc = cf = R.coef('A', M)
    B = T.Buffers(lib, M, False)
    if inputs is None:
        xb, g = T._rows(fp, D, M)
        inputs = (xb, R.make_batch(R.params(p), xb[:, :D], cf, g))
    xb, (acts, old_logp, adv, ret) = inputs
    scratch, out3 = fp._dw_buffers(16, M)
    out3.fill_(T.SENTINEL)
    ptr = T._ptr
    abi.check(lib.mas_policy_train_dw3(ptr(fp.packed), D, M, ptr(xb), fp.Dx, ptr(acts), ptr(old_logp), ptr(adv),
                                       ptr(ret), clip, vf, ec, sc, ptr(B.t['h1']), ptr(B.t['da1']), ptr(B.t['da2']),
                                       B.ld, ptr(B.part), ptr(out3), ptr(scratch), None))
    torch.cuda.synchronize()
    out = {k: raw(v) for k, v in B.t.items()}
    out['partials'] = raw(B.part)
    out['dw3_out'] = raw(out3)
    return out, inputs


def main(paths):
    if len(paths) < 2:
        sys.exit(__doc__)
    libs = [load(p) for p in paths]
    names = [os.path.basename(p) for p in paths]
    cases = [('train',) + c for c in T.CASES] + [('dw3', 'db', D, M, 'plain', 'A') for D, M in DW3_CASES]
    ndiff = 0
    for call, path, D, M, kind, cset in cases:
        M = M or T._grid_stride_rows()
        outs, inputs = [], None
        for lib in libs:
            mp = pytest.MonkeyPatch()
            try:
                if call == 'dw3':
                    o, inputs = dw3_outputs(lib, mp, D, M, inputs)
                else:
                    o, inputs = train_outputs(lib, mp, path, D, M, kind, cset, inputs)
            finally:
                mp.undo()
            outs.append(o)
        label = f'{call} {path} D={D} M={M} {kind} {cset}'
        nbytes = sum(v.numel() for v in outs[0].values())
        bad = []
        for name, o in zip(names[1:], outs[1:]):
            for k, v in outs[0].items():
                nd = int((v != o[k]).sum())
                if nd:
                    first = int((v != o[k]).nonzero()[0])
                    bad.append(f'{name} {k}: {nd} of {v.numel()} bytes differ, first at byte {first}')
        ndiff += len(bad)
        print(f'{label}: ' + (f'identical ({", ".join(outs[0])}; {nbytes} bytes)' if not bad
                              else 'DIFFERENT: ' + '; '.join(bad)), flush=True)
    print(f'{names[0]} vs {", ".join(names[1:])}: {len(cases)} cases, '
          + ('every buffer identical' if not ndiff else f'{ndiff} buffers differ'))
    return 1 if ndiff else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
