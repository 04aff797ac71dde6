"""The weighted PPO train kernels (mas_policy_train_w: the RW instantiations
of k_policy_train_db, k_policy_train_cw and k_policy_train) against the
unweighted ones on the same inputs, with the sentinel buffers and the batch of
test_gpu_policy_rows.py.  Three checks, none with a tolerance of its own:

1. w == 1 on every row: every buffer is bit-identical to mas_policy_train_ld's.
2. w in {0, 1}, about a third zeros: the rows with w = 1 are the unweighted
   call's rows; the rows with w = 0 are, as values, the rows of an unweighted
   call with adv = 0 and ent_coef = 0 (their policy terms vanish, their value
   term does not); the (v - ret)^2 partials are bit-identical, the clipped
   count is the reference's flags summed over the w = 1 rows, the surrogate
   and entropy sums lie within policy_rows_ref's partials bound of the fp64
   per-row terms times w; nothing outside the rows is written.
3. Garbage in the w = 0 rows (old_logp = -200: the ratio overflows; random
   actions; advantages of +-1e30): every output stays finite and equals check
   2's, the logit gradients of those rows still +-0."""
import ctypes

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import policy_rows_ref as R  # noqa: E402
import test_gpu_policy_rows as TR  # noqa: E402
from masurvival.abi import check  # noqa: E402

# (path, D, M); M = 0: the grid-stride size
CASES = [
    ('db', 160, 326), ('db', 138, 512), ('db', 160, 0),
    ('cw', 160, 326),
    ('plain', 160, 77), ('plain', 468, 130), ('plain', 138, 1),
    ('off64', 160, 326),
]
KEYS = ('h1', 'h2', 'dz', 'da2', 'da1')


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _run(B, fp, xb, batch, cf, w=None):
    """One call into the sentinel buffers B (refilled first); w: mas_policy_train_w.
    Returns clones of the raw buffers and partials."""
    B.refill()
    if w is None:
        B.run(fp, xb, batch, cf)
    else:
        acts, old_logp, adv, ret = batch
        clip, vf, ec, sc = cf
        t = B.t
        check(fp.lib.mas_policy_train_w(_ptr(fp.packed), fp.D, B.M, _ptr(xb), fp.Dx, _ptr(acts), _ptr(old_logp),
                                        _ptr(adv), _ptr(ret), _ptr(w), clip, vf, ec, sc, _ptr(t['h1']),
                                        _ptr(t['h2']), _ptr(t['da1']), _ptr(t['da2']), _ptr(t['dz']), B.ld,
                                        _ptr(B.part), None))
        torch.cuda.synchronize()
    assert B.untouched() == []
    raw = {k: v.clone() for k, v in B.t.items()}
    raw['part'] = B.part.clone()
    return raw


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


@pytest.mark.parametrize('path,D,M', CASES)
def test_weighted_train_rows(path, D, M, monkeypatch):
    M = M or TR._grid_stride_rows()
    TR._setenv(monkeypatch, path)
    p, fp = TR._policy(D, 'plain')
    assert hasattr(fp.lib, 'mas_policy_train_w')
    P = R.params(p)
    xb, g = TR._rows(fp, D, M)
    x = xb[:, :D]
    cf = R.coef('A', M)
    clip, vf, ec, sc = cf
    B = TR.Buffers(fp.lib, M, False)
    null = (torch.zeros((M, 6), dtype=torch.int8, device='cuda'),) + tuple(torch.zeros(M, device='cuda')
                                                                            for _ in range(3))
    B.run(fp, xb, null, cf)
    h2k = B.outputs(fp)['h2']
    batch = R.make_batch(P, x, cf, g, h2=h2k)
    acts, old_logp, adv, ret = batch
    U = _run(B, fp, xb, batch, cf)

    # 1. all ones
    W1 = _run(B, fp, xb, batch, cf, torch.ones(M, device='cuda'))
    for k in KEYS + ('part',):
        assert _same_bits(W1[k], U[k]), ('w == 1', k)

    # 2. zeros and ones
    w = (torch.rand(M, device='cuda', generator=g) >= 1.0 / 3.0).float()
    on, off = w != 0, w == 0
    Z = _run(B, fp, xb, (acts, old_logp, torch.zeros_like(adv), ret), (clip, vf, 0.0, sc))
    W = _run(B, fp, xb, batch, cf, w)
    for k in KEYS:
        assert _same_bits(W[k][:, :M][:, on], U[k][:, :M][:, on]), ('w = 1 rows', k)
        assert bool((W[k][:, :M][:, off].float() == Z[k][:, :M][:, off].float()).all()), ('w = 0 rows', k)
    assert bool((W['dz'][:15, :M][:, off].float() == 0.0).all())
    nb = B.nb
    assert _same_bits(W['part'][:nb, 1].contiguous(), U['part'][:nb, 1].contiguous())
    L = R.loss_rows(h2k.double() @ P['W3'].T + P['b3'], acts, old_logp, adv, ret, clip, vf, ec, sc)
    assert R.near_clip_rows(L['ratio'], clip) == 0
    wd = w.double()
    part = W['part'][:nb].double().sum(0)
    assert float(part[3]) == float((wd * L['clipped']).sum())
    for col, key in ((0, 'pg'), (2, 'ent')):
        d = abs(float(part[col] - (wd * L[key]).sum()))
        bound = R.FP32 * float((wd * L[key]).abs().sum())
        print(f'{path} D={D} M={M}: partials[{col}] |d| {d:.3g} bound {bound:.3g}')
        assert d <= bound, (key, d, bound)

    # 3. garbage where w = 0
    lp_g = torch.where(off, torch.full_like(old_logp, -200.0), old_logp)
    sign = torch.where(torch.rand(M, device='cuda', generator=g) < 0.5, -1.0, 1.0)
    adv_g = torch.where(off, 1e30 * sign, adv)
    hi = torch.tensor([3, 3, 3, 2, 2, 2], device='cuda')
    rnd = (torch.rand((M, 6), device='cuda', generator=g) * hi).long().clamp_(max=hi - 1).to(torch.int8)
    acts_g = torch.where(off[:, None], rnd, acts).contiguous()
    G = _run(B, fp, xb, (acts_g, lp_g.contiguous(), adv_g.contiguous(), ret), cf, w)
    for k in KEYS + ('part',):
        assert bool(torch.isfinite(G[k].float()).all()), ('finite', k)
    assert bool((G['dz'][:15, :M][:, off].float() == 0.0).all())
    for k in KEYS:
        assert _same_bits(G[k][:, :M][:, on], W[k][:, :M][:, on]), ('garbage, w = 1 rows', k)
        assert bool((G[k][:, :M][:, off].float() == W[k][:, :M][:, off].float()).all()), ('garbage, w = 0 rows', k)
    assert _same_bits(G['part'], W['part'])
