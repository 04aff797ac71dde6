"""The host restatement of the action sampler (tests/sampler_ref.py) on the
CPU: known answers that do not come from this repository, the extreme draws
(u = 1.0, u = 2^-25, two equal draws in one head), the statistics of the stream
at fixed seeds, the power of check_draws against a list of deliberate errors,
and the near-tie share of the reference alone.  test_gpu_act_rows.py holds the
kernels to this restatement row by row."""
import functools

import numpy as np
import pytest

import sampler_ref as S

BIG_SEED, BIG_STEP = 0xFEDCBA9876543210, (1 << 40) + 3

# upper 1e-3 points of chi-square at 3, 5 and 8 degrees of freedom (2x2, 2x3 and
# 3x3 tables against the uniform joint table; Abramowitz & Stegun table 26.8)
CHI2_CRIT = {3: 16.266, 5: 20.515, 8: 26.124}


def test_mix64_is_splitmix64():
    """The first two outputs of SplitMix64 seeded with 0 (the published
    vectors): its state after one and two steps is GOLDEN and 2 GOLDEN, and
    mix64 adds GOLDEN itself."""
    assert int(S.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(S.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4


def test_u_known_answers():
    xs = [0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 2, 2 ** 24 - 1]
    # x + 0.5 in fp32: exact below 2^23, to even above
    want = [2.0 ** -25, 3 * 2.0 ** -25, (2 ** 24 - 1) * 2.0 ** -25, 0.5, (2 ** 23 + 2) * 2.0 ** -24,
            (2 ** 24 - 2) * 2.0 ** -24, 1.0]
    u = S.u_from_x(xs)
    assert u.dtype == np.float32
    assert [float(v) for v in u] == want
    assert np.array_equal(S.u_from_r(np.asarray(xs, dtype=np.uint64) << np.uint64(40)), u)
    assert np.array_equal(S.u_from_r((np.asarray(xs, dtype=np.uint64) << np.uint64(40)) | np.uint64((1 << 40) - 1)), u)


@pytest.mark.parametrize('where', ['fused', 'sample'])
def test_extreme_tuples(where):
    ts = S.EXTREME[where]
    for kind, t in ts.items():
        seed, step, row, h, k = t
        assert 0 <= h < 6 and 0 <= k < S.HEAD_N[h]
        assert row < (4096 if where == 'sample' else 1 << 40)
        x = S.extreme_x(t)
        u = S.u_from_x(x)
        if kind == 'one':
            assert int(x[k]) == S.X_MAX and float(u[k]) == 1.0
        elif kind == 'min':
            assert int(x[k]) == 0 and float(u[k]) == S.U_MIN == 2.0 ** -25
        else:
            assert k + 1 < S.HEAD_N[h] and int(x[k]) == int(x[k + 1]) == int(x[:S.HEAD_N[h]].max())
        # the committed search finds the tuple in a window around it
        got = S.search_extreme(seed, step, 1, max(row - 500, 0), 1000, want=(kind,))
        assert got[kind][:3] == (seed, step, row)
    # u = 1.0: the score is +inf, the option wins against any logits, the log-prob is finite
    seed, step, row, h, k = ts['one']
    lg = np.zeros((1, 15), dtype=np.float32)
    lg[0, S.HEAD_OFF[h] + k] = -30.0
    u = S.stream_u(seed, step, row, 1)
    g, _ = S.scores(lg, u)
    assert g[0, h, k] == np.inf and not np.isnan(g).any()
    a = S.sample(lg, seed, step, row, 1)
    assert int(a[0, h]) == k
    lp, bound = S.log_prob(lg, a)
    assert np.isfinite(lp).all() and float(lp[0]) < -30.0
    res = S.check_draws(lg, seed, step, row, 1, a, lp.astype(np.float32))
    assert (res['wrong'], res['outside_top2'], res['range']) == (0, 0, 0) and res['logp'] <= 1.0, res
    # u = 2^-25: the largest penalty a draw can carry, log(25 ln 2)
    seed, step, row, h, k = ts['min']
    g, _ = S.scores(np.zeros((1, 15), dtype=np.float32), S.stream_u(seed, step, row, 1))
    assert abs(g[0, h, k] + np.log(25.0 * np.log(2.0))) < 1e-12 and g[0, h, k] == g[0][np.isfinite(g[0])].min()


# ---------------------------------------------------------------------------
# stream statistics

STAT_ROWS, STAT_SEED, STAT_STEP = 65536, 99, 3
LAGS = (1, 32, 64, 256)


def _chi2(a, b, na, nb):
    """(statistic, degrees of freedom) of the joint table of a and b against the uniform one."""
    t = np.bincount(a.astype(np.int64) * nb + b.astype(np.int64), minlength=na * nb).astype(np.float64)
    e = a.shape[0] / (na * nb)
    return float(((t - e) ** 2 / e).sum()), na * nb - 1


@functools.lru_cache(maxsize=None)
def _stream_stats(mut=None):
    """[(name, statistic, df)] and [(name, share of fully equal rows)]."""
    z = np.zeros((STAT_ROWS, 15), dtype=np.float32)
    a0 = S.sample(z, STAT_SEED, STAT_STEP, 0, STAT_ROWS, mut)
    other = {'step + 1': S.sample(z, STAT_SEED, STAT_STEP + 1, 0, STAT_ROWS, mut),
             'seed + 1': S.sample(z, STAT_SEED + 1, STAT_STEP, 0, STAT_ROWS, mut),
             'first_row 2^33': S.sample(z, STAT_SEED, STAT_STEP, 1 << 33, STAT_ROWS, mut)}
    assert int(a0.min()) == 0 and all(int(a0[:, h].max()) == n - 1 for h, n in enumerate(S.HEAD_N))
    chi, eq = [], []
    for i in range(6):
        for j in range(i + 1, 6):
            chi.append((f'heads {i}, {j}',) + _chi2(a0[:, i], a0[:, j], S.HEAD_N[i], S.HEAD_N[j]))
    for L in LAGS:
        for h, n in enumerate(S.HEAD_N):
            chi.append((f'head {h} lag {L}',) + _chi2(a0[:-L, h], a0[L:, h], n, n))
        eq.append((f'lag {L}', float((a0[:-L] == a0[L:]).all(1).mean())))
    for name, b in other.items():
        for h, n in enumerate(S.HEAD_N):
            chi.append((f'head {h} {name}',) + _chi2(a0[:, h], b[:, h], n, n))
        eq.append((name, float((a0 == b).all(1).mean())))
    return chi, eq


def _failures(mut):
    chi, eq = _stream_stats(mut)
    bad = [(n, s) for n, s, df in chi if s > CHI2_CRIT[df]]
    return bad + [(n, s) for n, s in eq if abs(s - 1.0 / 216.0) > 0.003]


def test_stream_statistics():
    """Zero logits (every option of a head equally likely), 65536 rows, seed 99,
    step 3: the joint table of every head pair, of each head with itself 1, 32,
    64 and 256 rows on, and with itself at step + 1, seed + 1 and first_row =
    2^33, against the uniform table at p >= 1e-3; the share of fully equal rows
    between two such streams within 0.003 of 1 / 216 (its standard deviation at
    65536 rows is 0.0003).  Deterministic."""
    chi, eq = _stream_stats()
    worst = max(chi, key=lambda c: c[1] / CHI2_CRIT[c[2]])
    print('worst chi-square', worst, 'of its 1e-3 point', CHI2_CRIT[worst[2]], '; equal rows', eq)
    try:
        from scipy.stats import chi2
        print('smallest p', min(float(chi2.sf(s, df)) for _, s, df in chi))
    except ImportError:
        pass
    assert len(chi) == 15 + 6 * (len(LAGS) + 3)
    assert _failures(None) == []


@pytest.mark.parametrize('mut', ['head_dropped', 'row_mod_32'])
def test_stream_statistics_reject_shared_draws(mut):
    bad = _failures(mut)
    print(mut, bad[:4])
    assert bad


# ---------------------------------------------------------------------------
# the power of check_draws

def _logits(M, scale, seed=5, cols=16):
    return (np.random.default_rng(seed).standard_normal((M, cols)) * scale).astype(np.float32)


# (M, first_row): the smallest many-row shapes of the GPU cases that the mutation can show at
SHAPE_FUSED = (133, 77)
SHAPE_SAMPLE = (255, 0)


def _mutated(lg, seed, step, first_row, M, mut):
    a = S.sample(lg, seed, step, first_row, M, mut)
    lp, _ = S.log_prob(lg, a)
    return S.check_draws(lg, seed, step, first_row, M, a, lp.astype(np.float32))


@pytest.mark.parametrize('M,first_row', [SHAPE_FUSED, SHAPE_SAMPLE])
def test_checker_passes_the_restatement(M, first_row):
    res = _mutated(_logits(M, 1.5), BIG_SEED, BIG_STEP, first_row, M, None)
    assert (res['wrong'], res['outside_top2'], res['range']) == (0, 0, 0), res
    assert res['logp'] <= 1.0 and res['near_share'] <= S.NEAR_CAP, res


# scan_ge has its own test; mas_sample_actions has no first_row to drop
@pytest.mark.parametrize('M,first_row,mut', [
    (M, fr, m) for M, fr in (SHAPE_FUSED, SHAPE_SAMPLE) for m in S.MUTATIONS
    if m != 'scan_ge' and not (m == 'first_row_dropped' and fr == 0)])
def test_checker_rejects_mutation(M, first_row, mut):
    res = _mutated(_logits(M, 1.5), BIG_SEED, BIG_STEP, first_row, M, mut)
    print(mut, M, res)
    assert res['wrong'] > 0, res
    if mut == 'third_logit_zero':
        assert res['range'] > 0, res


@pytest.mark.parametrize('where', ['fused', 'sample'])
def test_checker_rejects_ge_scan_at_a_forced_tie(where):
    """Zero logits at the row whose head draws the same u for two options: the
    two scores are equal in any precision and the strict scan keeps the lower
    index; a >= scan keeps the higher one and is counted wrong, not near."""
    seed, step, row, h, k = S.EXTREME[where]['tie']
    first_row, M = (row - 17, 33) if where == 'fused' else (0, 4099)
    lg = np.zeros((M, 16), dtype=np.float32)
    i = row - first_row
    assert int(S.sample(lg, seed, step, first_row, M)[i, h]) == k
    assert int(S.sample(lg, seed, step, first_row, M, 'scan_ge')[i, h]) == k + 1
    ok = _mutated(lg, seed, step, first_row, M, None)
    assert (ok['wrong'], ok['outside_top2']) == (0, 0), ok
    res = _mutated(lg, seed, step, first_row, M, 'scan_ge')
    assert res['wrong'] > 0, res


# ---------------------------------------------------------------------------
# the near-tie cap

@pytest.mark.parametrize('M', [4096, 65536])
@pytest.mark.parametrize('scale', [0.0, 1.5, 6.0])
def test_near_tie_share_of_random_logits(scale, M):
    s = S.near_share(_logits(M, scale), 1234, 7)
    print(f'randn x {scale}, {M} rows: near-tie share {s:.5f}')
    assert s <= S.NEAR_CAP


@pytest.mark.parametrize('M', [4096, 65536])
@pytest.mark.parametrize('kind', ['plain', 'x4', 'zero'])
def test_near_tie_share_of_policy_logits(kind, M):
    import torch

    import policy_rows_ref as R
    D = 160
    P = R.params(R.make_policy(D, kind))
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((M, D), generator=g) * 2.0).bfloat16()
    z = R.forward(P, x)[2].float().numpy()
    s = S.near_share(z, 1234, 7)
    print(f'policy {kind}, {M} rows: near-tie share {s:.5f}')
    assert s <= S.NEAR_CAP
