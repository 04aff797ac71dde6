"""The GAE checker itself (tests/gae_ref.py), without a GPU: the fp64
restatement on a case worked by hand and against masurvival.ppo.gae_reference,
the fp32 emulations of both kernel forms accepted by the bound at every T and
column edge the GPU test uses, every named mutation rejected, the exact case
bit-equal, and the normalisation / masked statistics restatements with their
clamps."""
import math

import numpy as np
import pytest

import gae_ref as G

torch = pytest.importorskip('torch')

from masurvival import ppo  # noqa: E402

F32 = np.float32
TS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 129, 150)
# (n_envs, n_agents): the column counts 1, 63, 64, 65, 255, 256, 257, 1025 and
# envs that straddle the 64- and 256-column workgroup edges (43 x 3, 86 x 3)
COLS = ((1, 1), (21, 3), (8, 8), (65, 1), (85, 3), (64, 4), (257, 1), (1025, 1), (43, 3), (86, 3), (32, 2))
HYPER = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0), (0.999, 0.99))


def f32pair(gamma, lam):
    return float(F32(gamma)), float(F32(lam))


def random_case(T, E, A, seed, p_done=0.05):
    rng = np.random.default_rng(seed)
    M = E * A
    r = rng.standard_normal((T, M)).astype(F32)
    v = rng.standard_normal((T + 1, M)).astype(F32)
    d = (rng.random((T, E)) < p_done).astype(np.uint8)
    return r, v, d


def test_known_answer_worked_by_hand():
    """T = 3, two envs of one agent, gamma = 1/2, lambda = 1/2 (c = 1/4).
    Column 0, no done: delta_2 = 1 + 4/2 - 2 = 1, delta_1 = 2 + 2/2 - 4 = -1,
    delta_0 = -1 + 4/2 - 0 = 1; A_2 = 1, A_1 = -1 + 1/4 = -3/4, A_0 = 1 -
    3/16 = 13/16.  Column 1, done at t = 1 (byte 255): delta_2 = 3 + 8/2 - 2
    = 5 = A_2; delta_1 = 1 - 6 = -5 = A_1 (nothing crosses the episode end);
    delta_0 = 2 + 6/2 - 1 = 4, A_0 = 4 - 5/4 = 11/4."""
    r = np.array([[-1, 2], [2, 1], [1, 3]], dtype=F32)
    v = np.array([[0, 1], [4, 6], [2, 2], [4, 8]], dtype=F32)
    d = np.array([[0, 0], [0, 255], [0, 0]], dtype=np.uint8)
    adv, ret = G.gae_ref(r, v, d, 0.5, 0.5, 1)
    assert adv.dtype == np.float64
    assert adv.tolist() == [[13 / 16, 11 / 4], [-3 / 4, -5.0], [1.0, 5.0]]
    assert ret.tolist() == [[13 / 16, 15 / 4], [13 / 4, 1.0], [3.0, 7.0]]
    # two agents per env: env 0's flag covers columns 0 and 1
    d2 = np.array([[0], [7], [0]], dtype=np.uint8)
    adv2, _ = G.gae_ref(r, v, d2, 0.5, 0.5, 2)
    assert adv2[1].tolist() == [2.0 - 4.0, -5.0] and adv2[0].tolist() == [1.0 - 2.0 / 4, 11 / 4]
    for form in G.FORMS:
        a, rt, _ = G.gae_emulate(form, r, v, d, 0.5, 0.5, 1)
        assert np.array_equal(a, adv) and np.array_equal(rt, ret)


@pytest.mark.parametrize('gamma,lam', HYPER)
def test_ppo_gae_reference_is_the_restatement_on_fp64(gamma, lam):
    T, E, A = 37, 11, 3
    r, v, d = random_case(T, E, A, 5, p_done=0.1)
    d[3, 2], d[9, 0], d[T - 1, 4], d[0, 5] = 2, 255, 128, 7   # nonzero bytes other than 1
    gamma, lam = f32pair(gamma, lam)
    adv, ret = G.gae_ref(r, v, d, gamma, lam, A)
    ta, tr = ppo.gae_reference(torch.from_numpy(r).double().reshape(T, E, A),
                               torch.from_numpy(v).double().reshape(T + 1, E, A), torch.from_numpy(d), gamma, lam, A)
    assert ta.dtype == torch.float64 and ta.shape == (T, E, A)
    for got, ref in ((ta, adv), (tr, ret)):
        got = got.reshape(T, -1).numpy()
        assert np.max(np.abs(got - ref) / (1.0 + np.abs(ref))) <= 1e-12


def _clean_cases():
    """Every T and every column configuration at least once, the
    hyperparameters in turn."""
    n = max(len(TS), len(COLS))
    for i in range(n):
        yield TS[i % len(TS)], COLS[i % len(COLS)], HYPER[i % len(HYPER)], i
    # the longest rollout at the widest trace, and every scan-chunk edge with agents > 1
    for i, T in enumerate((63, 64, 65, 128, 129, 150)):
        yield T, (43, 3), HYPER[4], 100 + i


def test_clean_emulations_are_accepted():
    worst = {f: 0.0 for f in G.FORMS}
    seen_t, seen_c = set(), set()
    for T, (E, A), (gamma, lam), seed in _clean_cases():
        seen_t.add(T)
        seen_c.add(E * A)
        gamma, lam = f32pair(gamma, lam)
        for kind in range(3):
            r, v, d = random_case(T, E, A, seed * 3 + kind, p_done=(0.05, 0.5, 0.0)[kind])
            if kind == 1:
                v += F32(1000.0)   # delta cancels
            if kind == 2:
                r *= F32(1e3)
            for form in G.FORMS:
                adv, ret, sums = G.gae_emulate(form, r, v, d, gamma, lam, A)
                q = G.check_gae(r, v, d, gamma, lam, A, adv, ret)
                s = G.check_sums(sums, adv)
                assert q['adv'] <= 1.0 and q['ret'] <= 1.0 and max(s) <= 1.0, (form, T, E, A, gamma, lam, kind, q, s)
                worst[form] = max(worst[form], q['adv'], q['ret'])
    assert seen_t == set(TS) and {1, 63, 64, 65, 255, 256, 257, 1025} <= seen_c
    print('clean emulations, worst |d| / bound: ' + ', '.join(f'{f} {w:.3f}' for f, w in worst.items()))
    assert min(worst.values()) > 0.01   # the bound is within two orders of the error it bounds


def _verdict(form, r, v, d, gamma, lam, A, mut):
    adv, ret, sums = G.gae_emulate(form, r, v, d, gamma, lam, A, mut=mut)
    q = G.check_gae(r, v, d, gamma, lam, A, adv, ret)
    written = np.where(np.isnan(adv), F32(0.0), adv)
    return max(q['adv'], q['ret'], *G.check_sums(sums, written)), adv, ret


MUT_CASES = [(m, f) for m, forms in G.MUTATIONS.items() for f in forms]


@pytest.mark.parametrize('mut,form', MUT_CASES)
def test_mutation(mut, form):
    """Each named error is rejected on random inputs (ratio > 1) -- T = 70
    has a scan carry and a walk tail of 6 steps, 43 envs x 3 agents a partial
    last workgroup in both forms -- except the rounding-level one, which the
    bound accepts by construction and the exact case tells apart exactly
    where it changes a bit."""
    T, E, A = 70, 43, 3
    gamma, lam = f32pair(0.99, 0.95)
    r, v, d = random_case(T, E, A, 11, p_done=0.05)
    clean, ca, cr = _verdict(form, r, v, d, gamma, lam, A, None)
    bad, ma, mr = _verdict(form, r, v, d, gamma, lam, A, mut)
    assert clean <= 1.0
    print(f'{form} {mut}: ratio {bad:.3g} (clean {clean:.3f})')
    xr, xv, xd = G.exact_case(T, E, A, 3)
    ref = G.gae_ref(xr, xv, xd, 0.5, 0.5, A)
    xa, xt, _ = G.gae_emulate(form, xr, xv, xd, 0.5, 0.5, A, mut=mut)
    exact_differs = not (np.array_equal(xa, ref[0]) and np.array_equal(xt, ref[1]))
    if mut in G.ROUNDING_LEVEL:
        # on the random inputs it does move bits, and stays inside the bound
        assert not np.array_equal(ma, ca) and bad <= 1.0
        # gamma lambda = 1/4 is exact: no bit moves, and the exact case agrees
        ka, kt, _ = G.gae_emulate(form, xr, xv, xd, 0.5, 0.5, A)
        changes_a_bit = not (np.array_equal(xa, ka) and np.array_equal(xt, kt))
        assert exact_differs == changes_a_bit and not changes_a_bit
        # where the product does round (1 + 2^-12 squared needs 25 bits) the
        # same integers differ from the kernel's arithmetic in some bit
        g2 = float(F32(1.0 + 2.0 ** -12))
        ya, _, _ = G.gae_emulate(form, xr, xv, xd, g2, g2, A, mut=mut)
        za, _, _ = G.gae_emulate(form, xr, xv, xd, g2, g2, A)
        assert not np.array_equal(ya, za)
        return
    assert bad > 1.0, (mut, form, bad)
    assert exact_differs or mut in ('sums_past_M',), (mut, form)   # (the sums are not part of the bit comparison)


@pytest.mark.parametrize('T,E,A', [(150, 70, 3), (129, 65, 1), (64, 8, 8), (9, 86, 3)])
def test_exact_case_is_bit_equal_for_both_emulations(T, E, A):
    r, v, d = G.exact_case(T, E, A, T + E)
    # no segment longer than 8 steps
    run = np.zeros(E, dtype=int)
    for t in range(T):
        run = np.where(d[t] != 0, 0, run + 1)
        assert run.max() < 8
    adv, ret = G.gae_ref(r, v, d, 0.5, 0.5, A)
    for form in G.FORMS:
        a, rt, sums = G.gae_emulate(form, r, v, d, 0.5, 0.5, A)
        assert np.array_equal(a.astype(np.float64), adv) and np.array_equal(rt.astype(np.float64), ret), form
        assert G.check_gae(r, v, d, 0.5, 0.5, A, a, rt)['adv'] == 0.0
        assert sums == (math.fsum(adv.ravel()), math.fsum((adv * adv).ravel()))   # exact sums too


def test_check_sums_rejects_a_dropped_term():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(5000).astype(F32)
    a64 = a.astype(np.float64)
    assert max(G.check_sums((np.sum(a64), np.sum(a64 * a64)), a)) <= 1.0
    assert max(G.check_sums((np.sum(a64[::-1]), np.sum((a64 * a64)[::-1])), a)) <= 1.0   # any order
    s = G.check_sums((np.sum(a64[:-1]), np.sum(a64 * a64)), a)
    assert s[0] > 1.0 and s[1] <= 1.0
    s = G.check_sums((np.sum(a64), np.sum((a64 * a64)[1:])), a)
    assert s[0] <= 1.0 and s[1] > 1.0
    # an fp32 accumulation is far outside
    assert G.check_sums((float(np.cumsum(a)[-1]), float(np.sum(a64 * a64))), a)[0] > 1.0


@pytest.mark.parametrize('shift', [0.0, 3.0, 1e4])
def test_adv_norm_ref_is_the_torch_expression_on_fp64(shift):
    rng = np.random.default_rng(int(shift))
    adv = (rng.standard_normal(1001) + shift).astype(F32)
    a64 = adv.astype(np.float64)
    stats = (float(a64.sum()), float((a64 * a64).sum()), float(adv.size))
    st = torch.tensor(stats, dtype=torch.float64)
    mean = st[0] / st[2]
    var = (st[1] / st[2] - mean * mean).clamp_min(0.0)
    # the trainer's expression, its two casts kept, everything else in double
    ref = (torch.from_numpy(a64) - mean.float().double()) / (var.sqrt().float() + 1e-8).double()
    out = G.adv_norm_ref(adv, stats)
    assert np.max(np.abs(out - ref.numpy()) / (1.0 + np.abs(ref.numpy()))) <= 1e-12
    # and the fp32 expression lies inside the bound
    got = torch.from_numpy(adv.copy()).sub_(mean.float()).div_(var.sqrt().float() + 1e-8).numpy()
    q = np.max(np.abs(got.astype(np.float64) - out) / G.adv_norm_bound(adv, stats))
    print(f'shift {shift}: torch fp32 expression at {q:.3f} of the bound')
    assert q <= 1.0
    # the statistics are taken as given: other statistics, another result
    other = G.adv_norm_ref(adv, (stats[0] + adv.size, stats[1], stats[2]))
    assert np.max(np.abs(other - out)) > 0.5


def test_adv_norm_ref_clamps_a_negative_variance():
    adv = np.full(8, 2.0, dtype=F32)
    stats = (16.0, 32.0 - 1e-9, 8.0)   # q / n - mean^2 = -1.25e-10
    out = G.adv_norm_ref(adv, stats)
    assert np.array_equal(out, np.zeros(8))
    out = G.adv_norm_ref(np.array([2.0 + 2.0 ** -20], dtype=F32), stats)
    assert out[0] == 2.0 ** -20 / float(F32(1e-8))   # sd = 0 + 1e-8f
    assert np.all(np.isfinite(G.adv_norm_bound(adv, stats)))


def test_masked_stats_ref_and_the_zero_count_clamp():
    rng = np.random.default_rng(2)
    adv = rng.standard_normal((4, 5, 3)).astype(F32)
    w = (rng.random((4, 5, 3)) < 0.5).astype(F32)
    s, q, n = G.masked_stats_ref(adv, w)
    a = adv.astype(np.float64)[w == 1.0]
    assert s == pytest.approx(a.sum(), rel=1e-14) and q == pytest.approx((a * a).sum(), rel=1e-14)
    assert n == float(w.sum()) >= 1.0
    assert G.masked_stats_ref(adv, np.zeros_like(w)) == (0.0, 0.0, 1.0)
    # the all-zero triple normalises to finite values: adv / 1e-8f
    out = G.adv_norm_ref(adv, (0.0, 0.0, 1.0))
    assert np.all(np.isfinite(out)) and np.array_equal(out, adv.astype(np.float64) / float(F32(1e-8)))
    with pytest.raises(AssertionError):
        G.masked_stats_ref(adv, w * 0.5)
