"""mas_policy_adam element by element against the fp64 restatement of
clip_grad_norm_ + torch.optim.Adam (tests/update_ref.py adam_ref), one step per
case within the bound check_adam derives from the kernel's fp32 roundings, on
flat buffers the test owns: a single element, a partial block (255), one
element into a second block (257), the last size of the first grid-stride pass
(131072 = 512 blocks of 256), three elements into the second pass (131075) and
the D = 468 policy's parameter count (189968), each with the clip active, off
(max_norm <= 0) and inactive, both gradient scales, step counts 1, 2, 7 and
1000, and every 7th gradient exactly 0.  Nothing past n is written, the
gradients are not written, and the scratch holds the partial sums of the
squared norm and nothing past its mas_policy_adam_scratch() floats.  The
figures measured on the MI355X are in profiles/update_check.txt."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import policy_rows_ref as R  # noqa: E402
import update_ref as UR  # noqa: E402
from masurvival.abi import check, load_library  # noqa: E402
from masurvival.ppo import FusedAdam, FusedPolicy  # noqa: E402

LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-5
PAD = 64            # sentinel floats past n
SENTINEL = -1234.0
SIZES = [1, 255, 257, 131072, 131075, 189968]
REGIMES = [(1, 0.5, 1.0), (2, 0.0, 1.0), (1000, 1e9, 0.125), (7, 0.5, 0.125)]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _state(n, step):
    """Host fp32 (p, g, m, v): random p; every 7th gradient exactly 0; both
    moments zero at step 1, else random with v >= 0."""
    r = np.random.default_rng(1000 * step + n)
    p = (0.1 * r.standard_normal(n)).astype(np.float32)
    g = (0.05 * r.standard_normal(n)).astype(np.float32)
    g[::7] = 0.0
    if step == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    g1 = 0.05 * r.standard_normal(n)
    return p, g, (0.3 * g1).astype(np.float32), (r.random(n) * g1 * g1).astype(np.float32)


def _padded(a):
    t = torch.full((a.shape[0] + PAD,), SENTINEL, dtype=torch.float32)
    t[:a.shape[0]] = torch.from_numpy(a)
    return t.cuda()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('step,max_norm,grad_scale', REGIMES)
def test_adam_step_matches_fp64_reference(n, step, max_norm, grad_scale):
    lib = load_library()
    ns = int(lib.mas_policy_adam_scratch())
    assert ns == 128
    p, g, m, v = _state(n, step)
    dp, dg, dm, dv = (_padded(a) for a in (p, g, m, v))
    scratch = torch.full((ns + PAD,), SENTINEL, dtype=torch.float32, device='cuda')
    check(lib.mas_policy_adam(n, _ptr(dp), _ptr(dg), _ptr(dm), _ptr(dv), grad_scale, max_norm, LR, BETAS[0],
                              BETAS[1], EPS, step, _ptr(scratch), None))
    torch.cuda.synchronize()
    hp, hg, hm, hv, hs = (t.cpu() for t in (dp, dg, dm, dv, scratch))
    for name, t in (('p', hp), ('g', hg), ('m', hm), ('v', hv)):
        assert bool((t[n:] == SENTINEL).all()), name + ': written past n'
    assert bool((hs[ns:] == SENTINEL).all()), 'scratch: written past mas_policy_adam_scratch() floats'
    assert torch.equal(hg[:n].view(torch.int32), torch.from_numpy(g).view(torch.int32)), 'g was written'
    # the scratch: the partial sums of |grad_scale g|^2, an fp32 sum of non-negative terms
    sq = float(np.sum((g.astype(np.float64) * grad_scale) ** 2))
    assert bool((hs[:ns] >= 0).all()) and abs(float(hs[:ns].double().sum()) - sq) <= R.FP32 * sq
    res = UR.check_adam(p, g, m, v, grad_scale, max_norm, LR, BETAS, EPS, step,
                        hp[:n].numpy(), hm[:n].numpy(), hv[:n].numpy())
    coef = UR._terms(p, g, m, v, grad_scale, max_norm, LR, BETAS, EPS, step)['coef']
    print(f'adam n={n} step={step} max_norm={max_norm:g} grad_scale={grad_scale:g} coef={coef:.3g}: '
          + ' '.join(f'{k} {res[k]:.3f}' for k in 'pmv'))
    for k in 'pmv':
        assert res[k] <= 1.0, (k, res)


def test_fused_adam_step_on_the_468_policy():
    """One FusedAdam.step on the D = 468 policy (189968 parameters: the kernel's
    second grid-stride pass) against adam_ref, and the torch.optim.Adam state
    reads back the same values through its views."""
    D = 468
    pol = R.make_policy(D).cuda()
    opt = torch.optim.Adam(pol.parameters(), lr=LR, betas=BETAS, eps=EPS)
    fa = FusedAdam(pol.parameters(), opt, FusedPolicy(pol, D, torch.device('cuda')).lib, torch.device('cuda'))
    n = fa.p.numel()
    assert n == 189968 == sum(q.numel() for q in pol.parameters())
    gen = torch.Generator(device='cuda').manual_seed(5)
    fa.g.copy_(0.05 * torch.randn(n, device='cuda', generator=gen))
    fa.g[::7] = 0.0
    p0, g0 = fa.p.cpu().numpy().copy(), fa.g.cpu().numpy().copy()
    assert bool((fa.m == 0).all()) and bool((fa.v == 0).all())
    fa.step(0.5)
    torch.cuda.synchronize()
    z = np.zeros(n, np.float32)
    p1, m1, v1 = fa.p.cpu().numpy(), fa.m.cpu().numpy(), fa.v.cpu().numpy()
    res = UR.check_adam(p0, g0, z, z, 1.0, 0.5, LR, BETAS, EPS, 1, p1, m1, v1)
    print('FusedAdam D=468 n=189968 step=1: ' + ' '.join(f'{k} {res[k]:.3f}' for k in 'pmv'))
    for k in 'pmv':
        assert res[k] <= 1.0, (k, res)
    assert np.array_equal(fa.g.cpu().numpy(), g0)
    off = 0
    for q in pol.parameters():
        st, k = opt.state[q], q.numel()
        assert float(st['step']) == 1.0
        assert st['exp_avg'].shape == q.shape and st['exp_avg_sq'].shape == q.shape
        assert np.array_equal(st['exp_avg'].detach().cpu().numpy().reshape(-1), m1[off:off + k])
        assert np.array_equal(st['exp_avg_sq'].detach().cpu().numpy().reshape(-1), v1[off:off + k])
        assert np.array_equal(q.detach().cpu().numpy().reshape(-1), p1[off:off + k])
        off += k
    assert off == n
    sd = opt.state_dict()['state']
    assert np.array_equal(torch.cat([sd[i]['exp_avg'].reshape(-1) for i in range(6)]).cpu().numpy(), m1)
