"""mas_gae (both forms: the per-column walk and the wavefront scan,
MAS_GAE_SCAN=1) and mas_adv_normalize element by element against the fp64
restatement of tests/gae_ref.py, within its derived bounds, at the shapes where
their index arithmetic can break: the edges of the walk's 8-step prefetch
chunk and of the scan's 64-step chunks (aligned from the end of the rollout),
the 64- and 256-column workgroup edges with envs that straddle them, more than
256 workgroups (the second pass of k_gae_sums), done flags placed on purpose,
and the exact case (gamma = lambda = 1/2 on integers), which both forms must
match bit for bit."""
import numpy as np
import pytest

import gae_ref as G

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import abi  # noqa: E402
from masurvival.ppo import adv_normalize, gae  # noqa: E402

F32 = np.float32
SENT, SENT_D = 12345.678, -7.25e300   # what the kernels must leave alone
TS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 129, 150)
# (n_envs, n_agents): 1, 63, 64, 65, 255, 256, 257, 1025 columns, and envs
# that straddle the 64- (43 x 3) and 256-column (86 x 3) workgroup edges
COLS = ((1, 1), (21, 3), (8, 8), (65, 1), (85, 3), (64, 4), (257, 1), (1025, 1), (43, 3), (86, 3), (32, 2))
PATTERNS = ('none', 'all', 'first', 'last', 'chunk_edges', 'p05', 'p50', 'bytes')
HYPER = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0), (0.999, 0.99))
KINDS = ('normal', 'shift1000', 'small_r', 'big_r')
# more than 256 workgroups in both forms (65538 columns: 257 of the walk's, 1025 of the scan's)
BIG = (9, (21846, 3))
WORST = {}


def _random_cases():
    out = []
    for i in range(2 * len(TS)):
        out.append((TS[i % len(TS)], COLS[(3 * i) % len(COLS)], PATTERNS[i % len(PATTERNS)], HYPER[i % len(HYPER)],
                    KINDS[(i // 2) % len(KINDS)]))
    # done flags either side of every scan chunk boundary, agents straddling the column edges
    out += [(T, (43, 3), 'chunk_edges', HYPER[i % 2], 'normal') for i, T in enumerate((65, 128, 129, 150))]
    out += [(150, (86, 3), 'p05', HYPER[4], 'normal'), (129, (64, 4), 'bytes', HYPER[0], 'shift1000'),
            (64, (8, 8), 'last', HYPER[4], 'big_r'), (17, (32, 2), 'first', HYPER[1], 'small_r'),
            BIG + ('p05', HYPER[0], 'normal')]
    return out


RANDOM_CASES = _random_cases()
EXACT_CASES = [(T, COLS[(3 * i) % len(COLS)]) for i, T in enumerate(TS)] + [(150, (70, 3)), (65, (86, 3)), BIG]


def _dones(pattern, T, E, rng):
    d = np.zeros((T, E), dtype=np.uint8)
    half = lambda: np.concatenate([[True], rng.random(E - 1) < 0.5])  # noqa: E731  (env 0 always)
    if pattern == 'all':
        d[:] = 1
    elif pattern == 'first':
        d[0, half()] = 1
    elif pattern == 'last':
        d[T - 1, half()] = 1
    elif pattern == 'chunk_edges':
        for k in (64, 65, 128, 129):
            if T - k >= 0:
                d[T - k, half()] = 1
    elif pattern in ('p05', 'p50'):
        d[rng.random((T, E)) < (0.05 if pattern == 'p05' else 0.5)] = 1
    elif pattern == 'bytes':
        on = rng.random((T, E)) < 0.2
        d[on] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=int(on.sum()))
    else:
        assert pattern == 'none'
    return d


def _inputs(T, E, A, pattern, kind, seed):
    rng = np.random.default_rng(seed)
    M = E * A
    r = rng.standard_normal((T, M)).astype(F32)
    v = rng.standard_normal((T + 1, M)).astype(F32)
    if kind == 'shift1000':
        v += F32(1000.0)
    elif kind == 'small_r':
        r *= F32(1e-3)
    elif kind == 'big_r':
        r *= F32(1e3)
    return r, v, _dones(pattern, T, E, rng)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64 if t.dtype == torch.float64
                               else torch.uint8)


def _run(form, r, v, d, gamma, lam, A, monkeypatch):
    """One mas_gae call of the form, twice, on interior views of larger
    sentinel-filled tensors: (adv, ret float32 [T][M], sums) as numpy, after
    the checks that hold for every case: inputs and sentinels bit-unchanged,
    the scratch untouched past its stated size, the sums identical from call
    to call."""
    monkeypatch.setenv('MAS_GAE_SCAN', '1' if form == 'scan' else '0')
    T, M = r.shape
    tr, tv, td = (torch.from_numpy(x).cuda() for x in (r, v, d))
    keep = [x.clone() for x in (tr, tv, td)]
    n_scr = abi.load_library().mas_gae_scratch_doubles(M)
    assert n_scr == 2 * ((M + 63) // 64)
    outs = []
    for call in range(2):
        adv_big = torch.full((T + 2, M), SENT, device='cuda')
        ret_big = torch.full((T + 2, M), SENT, device='cuda')
        sums_big = torch.full((4,), SENT_D, device='cuda', dtype=torch.float64)
        scratch = torch.full((n_scr + 16,), SENT_D, device='cuda', dtype=torch.float64)
        gae(tr, tv, td, gamma, lam, adv_big[1:T + 1], ret_big[1:T + 1], sums_big[1:3], A, scratch=scratch)
        torch.cuda.synchronize()
        for big in (adv_big, ret_big):
            assert bool((big[0] == SENT).all()) and bool((big[T + 1] == SENT).all()), 'a row outside [0, T) written'
        assert sums_big[0] == SENT_D and sums_big[3] == SENT_D
        assert bool((scratch[n_scr:] == SENT_D).all()), 'scratch written past mas_gae_scratch_doubles'
        outs.append((adv_big[1:T + 1].clone(), ret_big[1:T + 1].clone(), sums_big[1:3].clone()))
    for x, k in zip((tr, tv, td), keep):
        assert torch.equal(_bits(x), _bits(k)), 'an input changed'
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b)), 'two calls on the same inputs differ'
    adv, ret, sums = outs[0]
    return adv.cpu().numpy(), ret.cpu().numpy(), sums.cpu().numpy()


def _note(family, q):
    WORST[family] = max(WORST.get(family, 0.0), q)


@pytest.mark.parametrize('form', G.FORMS)
@pytest.mark.parametrize('T,cols,pattern,hyper,kind', RANDOM_CASES,
                         ids=[f'T{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-{c[3][0]}_{c[3][1]}-{c[4]}' for c in RANDOM_CASES])
def test_gae_within_the_bound(T, cols, pattern, hyper, kind, form, monkeypatch):
    (E, A), gamma, lam = cols, float(F32(hyper[0])), float(F32(hyper[1]))
    r, v, d = _inputs(T, E, A, pattern, kind, seed=1000 * T + E)
    adv, ret, sums = _run(form, r, v, d, gamma, lam, A, monkeypatch)
    q = G.check_gae(r, v, d, gamma, lam, A, adv, ret)
    s = G.check_sums(sums, adv)
    print(f'{form}: adv {q["adv"]:.3f} ret {q["ret"]:.3f} of the bound (worst at {q["at"]}), '
          f'sums {s[0]:.3f} {s[1]:.3f}')
    _note(f'{form} adv', q['adv'])
    _note(f'{form} ret', q['ret'])
    _note(f'{form} sums', max(s))
    assert q['adv'] <= 1.0 and q['ret'] <= 1.0, q
    assert max(s) <= 1.0, s


@pytest.mark.parametrize('T,cols', EXACT_CASES, ids=[f'T{c[0]}-{c[1][0]}x{c[1][1]}' for c in EXACT_CASES])
def test_exact_case_is_bit_equal_to_fp64_in_both_forms(T, cols, monkeypatch):
    E, A = cols
    r, v, d = G.exact_case(T, E, A, seed=T + E)
    ra, rr = G.gae_ref(r, v, d, 0.5, 0.5, A)
    got = {}
    for form in G.FORMS:
        adv, ret, sums = _run(form, r, v, d, 0.5, 0.5, A, monkeypatch)
        bad = np.argwhere(adv.astype(np.float64) != ra)
        assert bad.size == 0, (form, 'adv', len(bad), bad[:4].tolist())
        assert np.array_equal(ret.astype(np.float64), rr), (form, 'ret')
        s = G.check_sums(sums, adv)
        _note(f'{form} sums', max(s))
        assert max(s) <= 1.0, (form, s)
        got[form] = (adv, ret)
    for a, b in zip(got['walk'], got['scan']):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('form', G.FORMS)
def test_masking_is_a_product_by_zero(form, monkeypatch):
    """include/masurvival.h: the done flag multiplies by zero, so a
    non-finite masked value still propagates.  An infinite bootstrap value
    under a done last step makes that column's advantages NaN all the way
    back (through every earlier episode end as well); the other columns are
    as without it."""
    T, E, A = 20, 5, 3
    r, v, d = _inputs(T, E, A, 'p05', 'normal', seed=9)
    d[T - 1, 2] = 1
    d[7, 2] = 1
    col = 2 * A + 1
    v[T, col] = np.inf
    gamma, lam = float(F32(0.99)), float(F32(0.95))
    adv, ret, _ = _run(form, r, v, d, gamma, lam, A, monkeypatch)
    assert np.all(np.isnan(adv[:, col])) and np.all(np.isnan(ret[:, col]))
    others = np.arange(E * A) != col
    v[T, col] = 0.0
    ra, rr, ba, br = G.gae_ref_and_bound(r, v, d, gamma, lam, A)
    assert np.all(np.abs(adv - ra)[:, others] <= ba[:, others]) and np.all(np.abs(ret - rr)[:, others] <= br[:, others])


NORM_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099)


@pytest.mark.parametrize('shift', [0.0, 3.0, 1e4])
@pytest.mark.parametrize('n', NORM_N)
def test_adv_normalize_within_the_bound(n, shift):
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) + shift).astype(F32)
    a64 = a.astype(np.float64)
    stats = (float(np.sum(a64)), float(np.sum(a64 * a64)), float(n))
    big = torch.full((n + 12,), SENT, device='cuda')
    out = big[4:4 + n]          # 16 bytes in: aligned, sentinels on both sides
    out.copy_(torch.from_numpy(a))
    st = torch.tensor(stats, dtype=torch.float64, device='cuda')
    adv_normalize(out, st)
    torch.cuda.synchronize()
    assert bool((big[:4] == SENT).all()) and bool((big[4 + n:] == SENT).all()), 'written outside [0, n)'
    assert st.tolist() == list(stats)
    got = out.cpu().numpy().astype(np.float64)
    q = float(np.max(np.abs(got - G.adv_norm_ref(a, stats)) / G.adv_norm_bound(a, stats)))
    print(f'n {n} shift {shift}: {q:.3f} of the bound')
    _note('adv_normalize', q)
    assert q <= 1.0


def test_adv_normalize_zero_variance_clamp_and_zero_count_triple():
    a = np.full(8, 2.0, dtype=F32)
    stats = (16.0, 32.0 - 1e-9, 8.0)   # q / n - mean^2 < 0: clamped, sd = 1e-8f
    out = torch.from_numpy(a).cuda()
    adv_normalize(out, torch.tensor(stats, dtype=torch.float64, device='cuda'))
    assert np.array_equal(out.cpu().numpy(), G.adv_norm_ref(a, stats).astype(F32)) and not out.any()
    # the triple of a rollout without an active row: (0, 0, 1)
    b = np.random.default_rng(0).standard_normal(37).astype(F32)
    out = torch.from_numpy(b).cuda()
    adv_normalize(out, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device='cuda'))
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - G.adv_norm_ref(b, (0.0, 0.0, 1.0))) <= G.adv_norm_bound(b, (0.0, 0.0, 1.0)))


def test_the_case_tables_cover_every_listed_value_and_report():
    ts = {c[0] for c in RANDOM_CASES}
    cols = {c[1][0] * c[1][1] for c in RANDOM_CASES}
    assert ts == set(TS) and {c[0] for c in EXACT_CASES} >= set(TS)
    assert {1, 63, 64, 65, 255, 256, 257, 1025} <= cols and {1, 2, 3, 4, 8} == {c[1][1] for c in RANDOM_CASES}
    assert {1, 63, 64, 65, 255, 256, 257, 1025} <= {c[1][0] * c[1][1] for c in EXACT_CASES}
    assert {c[2] for c in RANDOM_CASES} == set(PATTERNS) and {c[3] for c in RANDOM_CASES} == set(HYPER)
    assert {c[4] for c in RANDOM_CASES} == set(KINDS)
    assert BIG[1][0] * BIG[1][1] > 65536   # more than 256 workgroups of either form
    print('worst |d| / bound per family: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))
