"""mas_gae_scaled in both forms (the per-column walk and the wavefront scan,
MAS_GAE_SCAN=1) against mas_gae itself, bit for bit: with a scale of 1 and no
clip on the same rewards, and with a scale and a clip that bites at both ends
on torch.clamp(r * s, -c, c).  The shapes are those of test_gpu_gae_rows.py
that sit on the walk's 8-step chunk edge, the scan's 64-step chunk edge and
the 64- and 256-column workgroup edges (with envs that straddle them).  The
rewards are not written, and the scale is read from device memory."""
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import gae, gae_scaled  # noqa: E402

F32 = np.float32
FORMS = ('walk', 'scan')
# (T, (n_envs, n_agents)): T around 8 and around 64 (and two scan chunks + 1);
# 63, 65, 255, 256, 257 columns, envs across the 64- (43 x 3) and 256-column (86 x 3) edges
CASES = ((7, (21, 3)), (8, (65, 1)), (9, (85, 3)), (63, (64, 4)), (64, (257, 1)), (65, (43, 3)), (129, (86, 3)),
         (16, (8, 8)))
GAMMA, LAM = float(F32(0.99)), float(F32(0.95))


def _inputs(T, E, A, seed):
    rng = np.random.default_rng(seed)
    M = E * A
    r = (8.0 * rng.standard_normal((T, M))).astype(F32)   # r * 0.37 has a deviation near 3: 1.5 clips both ends
    v = rng.standard_normal((T + 1, M)).astype(F32)
    d = (rng.random((T, E)) < 0.1).astype(np.uint8)
    d[d != 0] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=int((d != 0).sum()))
    return tuple(torch.from_numpy(x).cuda() for x in (r, v, d))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _outs(T, M):
    return (torch.full((T, M), 7.5, device='cuda'), torch.full((T, M), 7.5, device='cuda'),
            torch.full((2,), -1.0, device='cuda', dtype=torch.float64))


def _plain(r, v, d, A):
    o = _outs(*r.shape)
    gae(r, v, d, GAMMA, LAM, o[0], o[1], o[2], A)
    return o


def _scaled(r, v, d, A, scale, clip):
    o = _outs(*r.shape)
    gae_scaled(r, v, d, GAMMA, LAM, scale, clip, o[0], o[1], o[2], A)
    return o


def _same(a, b, what):
    for x, y, name in zip(a, b, ('adv', 'ret', 'sums')):
        assert torch.equal(_bits(x), _bits(y)), (what, name, int((_bits(x) != _bits(y)).sum()))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('T,cols', CASES, ids=[f'T{c[0]}-{c[1][0]}x{c[1][1]}' for c in CASES])
def test_scaled_is_mas_gae_on_the_scaled_and_clamped_rewards(T, cols, form, monkeypatch):
    monkeypatch.setenv('MAS_GAE_SCAN', '1' if form == 'scan' else '0')
    E, A = cols
    r, v, d = _inputs(T, E, A, seed=100 * T + E)
    keep = r.clone()
    # a scale of 1 and no clip: mas_gae's bits
    one = torch.ones((1,), device='cuda')
    _same(_scaled(r, v, d, A, one, math.inf), _plain(r, v, d, A), 'identity')
    # a scale and a clip that bites at both ends (the product an fp32 rounding of its own)
    s = torch.tensor([0.37], device='cuda')
    copy = torch.clamp(r * s, -1.5, 1.5)
    if r.numel() >= 60:
        assert bool((copy == 1.5).any()) and bool((copy == -1.5).any()) and bool((copy.abs() < 1.5).any())
    got = _scaled(r, v, d, A, s, 1.5)
    _same(got, _plain(copy, v, d, A), 'scaled')
    assert bool(torch.isfinite(got[0]).all()) and not torch.equal(got[0], _plain(r, v, d, A)[0])
    assert torch.equal(_bits(r), _bits(keep)), 'the rewards were written'
    assert s.tolist() == [F32(0.37)]


@pytest.mark.parametrize('form', FORMS)
def test_scale_is_read_from_the_device_at_run_time(form, monkeypatch):
    """The scale changes between two calls by a device-side write, with no
    host synchronisation in between: each call sees the value stream order
    gives it."""
    monkeypatch.setenv('MAS_GAE_SCAN', '1' if form == 'scan' else '0')
    T, (E, A) = 17, (86, 3)
    r, v, d = _inputs(T, E, A, seed=4)
    s = torch.tensor([0.37], device='cuda')
    factor = torch.tensor([0.25], device='cuda')
    a = _scaled(r, v, d, A, s, 1.5)
    s.mul_(factor)                       # stream-ordered, the host does not wait
    b = _scaled(r, v, d, A, s, 1.5)
    torch.cuda.synchronize()
    s1 = torch.tensor([0.37], device='cuda')
    _same(a, _plain(torch.clamp(r * s1, -1.5, 1.5), v, d, A), 'first call')
    _same(b, _plain(torch.clamp(r * (s1 * factor), -1.5, 1.5), v, d, A), 'second call')
    assert not torch.equal(a[0], b[0])


@pytest.mark.parametrize('form', FORMS)
def test_a_nan_reward_passes_the_clamp_and_infinities_are_clipped(form, monkeypatch):
    monkeypatch.setenv('MAS_GAE_SCAN', '1' if form == 'scan' else '0')
    T, (E, A) = 9, (21, 3)
    r, v, d = _inputs(T, E, A, seed=6)
    d.zero_()
    r[5, 7] = math.nan
    r[3, 11] = math.inf
    r[4, 12] = -math.inf
    s = torch.tensor([0.37], device='cuda')
    adv, ret, _ = _scaled(r, v, d, A, s, 1.5)
    assert bool(torch.isnan(adv[:6, 7]).all()) and bool(torch.isfinite(adv[6:, 7]).all())
    want = _plain(torch.clamp(r * s, -1.5, 1.5), v, d, A)
    others = torch.arange(E * A, device='cuda') != 7
    assert torch.equal(_bits(adv[:, others]), _bits(want[0][:, others]))
    assert torch.equal(_bits(ret[:, others]), _bits(want[1][:, others]))
    assert bool(torch.isfinite(adv[:, 11]).all()) and bool(torch.isfinite(adv[:, 12]).all())
