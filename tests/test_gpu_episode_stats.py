"""mas_episode_stats against the restatement
(masurvival.ppo.episode_stats_reference, held to the plain loop of
tests/ep_ref.py by tests/test_episode_stats_reference.py) at the shapes where
its index arithmetic can break: the edges of the prefetch chunk, the workgroup
edge, every agent count of the template, more workgroups than the final sum
has threads (its strided second pass), done flags placed on purpose, four kinds
of side mask, carries that are not zero going in.

Two reward families.  Half-integers in [-1, 1]: every sum is exact in fp64, so
the whole record and both carries must equal the restatement exactly; this is
what pins wins and draws.  standard_normal fp32: ret_carry has one order of
operations and is held bit for bit, len_carry and the integer entries are
exact, and sum_G / sum_G2 are held to n 2^-53 sum|G| / (n + 1) 2^-53 sum G^2
around the math.fsum totals of the plain loop's per-episode returns (the
derivation in tests/ep_ref.py)."""
import functools

import numpy as np
import pytest

import ep_ref as R

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import abi  # noqa: E402
from masurvival.ppo import (EPISODE_STATS_CHUNK as CH, EpisodeStats, episode_stats,  # noqa: E402
                            episode_stats_geometry, episode_stats_reference)

WG, MAX_AGENTS = episode_stats_geometry()  # of the loaded library

F32 = np.float32
SENT_D, SENT_I = -7.25e300, -123456789   # what the kernel must leave alone
TS = (1, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1, 64, 65)
EAS = ((1, 1), (21, 3), (64, 4), (65, 4), (86, 3), (257, 1), (33, 8), (40, 5), (50, 7))
BIG = (257 * WG + 1, 2)  # more workgroups than k_ep_sums has threads
PATTERNS = ('none', 'all', 'first', 'last', 'p05', 'p50', 'bytes')
MASKS = ('none', 'full', 'lower', 'inter')
FAMILIES = ('half', 'normal')
# (T, (E, A), side mask, pattern) with two sides, kept in the table on purpose: short episodes of few agents draw
PINNED = ((CH + 1, (64, 4), 0b0011, 'p05'), (2 * CH, (86, 3), 0b101, 'p50'), (CH, (33, 8), 0x0F, 'p05'),
          (2 * CH + 1, (65, 4), 0b0101, 'all'), (CH - 1, (40, 5), 0b00011, 'bytes'), (65, (50, 7), 0b1010101, 'last'),
          (CH + 1, (64, 2), 0b01, 'p50'), (CH, (30, 6), 0b000111, 'p50'))
WORST = {}


def _mask(kind, A):
    full = (1 << A) - 1
    return {'none': 0, 'full': full, 'lower': (1 << (A // 2)) - 1, 'inter': 0b01010101 & full}[kind]


def _cases():
    out = []
    for i in range(4 * len(TS)):
        E, A = EAS[(5 * i) % len(EAS)]
        out.append((TS[i % len(TS)], (E, A), _mask(MASKS[(i + i // 4) % len(MASKS)], A), PATTERNS[i % len(PATTERNS)]))
    out += list(PINNED)
    out += [(CH + 1, BIG, 0b01, 'p05'), (1, BIG, 0b10, 'all')]
    return out


CASES = _cases()
IDS = [f'T{c[0]}-{c[1][0]}x{c[1][1]}-m{c[2]:x}-{c[3]}' for c in CASES]


def _dones(pattern, T, E, rng):
    d = np.zeros((T, E), dtype=np.uint8)
    half = lambda: np.concatenate([[True], rng.random(E - 1) < 0.5])  # noqa: E731  (env 0 always)
    if pattern == 'all':
        d[:] = 1
    elif pattern == 'first':
        d[0, half()] = 1
    elif pattern == 'last':
        d[T - 1, half()] = 1
    elif pattern in ('p05', 'p50'):
        d[rng.random((T, E)) < (0.05 if pattern == 'p05' else 0.5)] = 1
    elif pattern == 'bytes':
        on = rng.random((T, E)) < 0.2
        d[on] = rng.choice(np.array([2, 255], dtype=np.uint8), size=int(on.sum()))
    else:
        assert pattern == 'none'
    return d


@functools.lru_cache(maxsize=None)
def _inputs(T, ea, pattern, family):
    """(rewards [T, E*A] fp32, dones [T, E] uint8, ret_carry fp64, len_carry int32): non-zero carries going in."""
    E, A = ea
    rng = np.random.default_rng(1000 * T + 7 * E + A + (0 if family == 'half' else 500000))
    if family == 'half':
        r = (rng.integers(-2, 3, size=(T, E * A)) * 0.5).astype(F32)
        G = rng.integers(-6, 7, size=E * A) * 0.5
        G[G == 0] = 0.5
    else:
        r = rng.standard_normal((T, E * A)).astype(F32)
        G = 3.0 * rng.standard_normal(E * A)
    ln = rng.integers(1, 40, size=E).astype(np.int32)
    return r, _dones(pattern, T, E, rng), G.astype(np.float64), ln


@functools.lru_cache(maxsize=None)
def _restate(T, ea, mask, pattern, family):
    r, d, G, ln = _inputs(T, ea, pattern, family)
    g, n, rec = episode_stats_reference(torch.from_numpy(r), torch.from_numpy(d), ea[1], torch.from_numpy(G),
                                        torch.from_numpy(ln), mask)
    return g.numpy(), n.numpy(), rec.numpy()


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _run(r, d, G, ln, A, mask):
    """mas_episode_stats twice from the same carries, on interior views of
    larger sentinel-filled tensors and with different scratch contents:
    (ret_carry, len_carry, record) as numpy, after the checks every case shares."""
    T, M = r.shape
    E, NV = M // A, 6 + 2 * A
    tr, td = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    keep = [x.clone() for x in (tr, td)]
    n_scr = abi.load_library().mas_episode_stats_scratch_doubles(E, A)
    assert n_scr == NV * ((E + WG - 1) // WG)
    outs = []
    for fill in (SENT_D, 3.5e11):
        g_big = torch.full((M + 8,), SENT_D, device='cuda', dtype=torch.float64)
        g_big[4:4 + M].copy_(torch.from_numpy(G))
        l_big = torch.full((E + 8,), SENT_I, device='cuda', dtype=torch.int32)
        l_big[4:4 + E].copy_(torch.from_numpy(ln))
        rec_big = torch.full((NV + 4,), SENT_D, device='cuda', dtype=torch.float64)
        scratch = torch.full((n_scr + 16,), fill, device='cuda', dtype=torch.float64)
        episode_stats(tr, td, A, g_big[4:4 + M], l_big[4:4 + E], rec_big[2:2 + NV], side_mask=mask, scratch=scratch)
        torch.cuda.synchronize()
        assert bool((g_big[:4] == SENT_D).all()) and bool((g_big[4 + M:] == SENT_D).all()), 'ret_carry overrun'
        assert bool((l_big[:4] == SENT_I).all()) and bool((l_big[4 + E:] == SENT_I).all()), 'len_carry overrun'
        assert bool((rec_big[:2] == SENT_D).all()) and bool((rec_big[2 + NV:] == SENT_D).all()), 'record overrun'
        assert bool((scratch[n_scr:] == fill).all()), 'scratch written past mas_episode_stats_scratch_doubles'
        outs.append((g_big[4:4 + M].clone(), l_big[4:4 + E].clone(), rec_big[2:2 + NV].clone()))
    for x, k in zip((tr, td), keep):
        assert torch.equal(_bits(x), _bits(k)), 'an input changed'
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b)), 'two calls with different scratch contents differ'
    return tuple(x.cpu().numpy() for x in outs[0])


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('T,ea,mask,pattern', CASES, ids=IDS)
def test_kernel_against_the_restatement(T, ea, mask, pattern, family):
    E, A = ea
    r, d, G, ln = _inputs(T, ea, pattern, family)
    got_G, got_len, got_rec = _run(r, d, G, ln, A, mask)
    want_G, want_len, want_rec = _restate(T, ea, mask, pattern, family)
    bad = np.argwhere(got_G.view(np.int64) != want_G.view(np.int64))
    assert bad.size == 0, ('ret_carry', len(bad), bad[:4].tolist())
    assert np.array_equal(got_len, want_len), 'len_carry'
    assert got_rec[:6].tolist() == want_rec[:6].tolist(), (got_rec[:6], want_rec[:6])
    if mask in (0, (1 << A) - 1):
        assert got_rec[3:6].tolist() == [0, 0, 0]
    if family == 'half':
        assert got_rec.tolist() == want_rec.tolist(), (got_rec, want_rec)  # every sum is exact
        return
    _, _, c, ep = R.walk(r, d, A, G, ln, mask)
    assert got_rec[:6].tolist() == [float(c[k]) for k in R.HEAD]
    q = R.check_sums(got_rec, c, ep)
    print(f'sums {q:.3f} of the bound ({c["episodes"]} episodes)')
    WORST['sums'] = max(WORST.get('sums', 0.0), q)
    assert q <= 1.0, (q, got_rec, want_rec)
    assert R.check_sums(want_rec, c, ep) <= 1.0  # the restatement itself, on this case


def test_two_rollouts_chain_through_the_carries():
    """Rows [0, 9) then [9, 26) from the first call's carries: the carries of
    one call over all 26 rows bit for bit, integer entries that add up."""
    A, mask = 3, 0b011
    r, d, G, ln = _inputs(26, (86, 3), 'p05', 'normal')
    g_all, n_all, rec_all = _run(r, d, G, ln, A, mask)
    g_a, n_a, rec_a = _run(r[:9].copy(), d[:9].copy(), G, ln, A, mask)
    g_b, n_b, rec_b = _run(r[9:].copy(), d[9:].copy(), g_a, n_a, A, mask)
    assert np.array_equal(g_b.view(np.int64), g_all.view(np.int64)) and np.array_equal(n_b, n_all)
    assert (rec_a[:6] + rec_b[:6]).tolist() == rec_all[:6].tolist() and rec_all[0] > 0
    _, _, c, ep = R.walk(r, d, A, G, ln, mask)
    assert R.check_sums(rec_a + rec_b, c, ep) <= 2.0  # two partial sums and the addition here


def test_the_half_integer_cases_count_wins_of_both_sides_and_draws():
    """The condition that keeps the exact comparison from passing vacuously: by
    the restatement alone, over the half-integer cases with two sides."""
    w0 = w1 = dr = 0
    for T, ea, mask, pattern in CASES:
        if mask in (0, (1 << ea[1]) - 1) or ea == BIG:
            continue
        rec = _restate(T, ea, mask, pattern, 'half')[2]
        print(f'T {T}, {ea[0]} x {ea[1]}, mask {mask:#x}, {pattern}: {int(rec[3])}, {int(rec[4])} wins, '
              f'{int(rec[5])} draws of {int(rec[0])}')
        w0, w1, dr = w0 + rec[3], w1 + rec[4], dr + rec[5]
    assert w0 >= 1 and w1 >= 1 and dr >= 1, (w0, w1, dr)
    for T, ea, mask, pattern in PINNED[1:2] + PINNED[-2:]:  # each of these alone has all three
        rec = _restate(T, ea, mask, pattern, 'half')[2]
        assert min(rec[3:6]) >= 1, (T, ea, mask, pattern, rec[:6])


def test_wrapper_refusals_and_the_case_table():
    r = torch.zeros((4, 6), device='cuda')
    d = torch.zeros((4, 2), dtype=torch.uint8, device='cuda')
    g = torch.zeros((6,), dtype=torch.float64, device='cuda')
    n = torch.zeros((2,), dtype=torch.int32, device='cuda')
    rec = torch.full((12,), 5.0, dtype=torch.float64, device='cuda')
    episode_stats(r, d, 3, g, n, rec, side_mask=0b001)
    torch.cuda.synchronize()
    assert rec.tolist() == [0.0] * 12 and not g.any() and n.tolist() == [4, 4]
    for bad in (dict(g=g[:5]), dict(g=g.float()), dict(n=n.long()), dict(n=n[:1]), dict(rec=rec[:11]),
                dict(rec=rec.float()), dict(d=d.float()), dict(A=2), dict(mask=0b1000), dict(g=g.cpu()),
                dict(scratch=torch.zeros((1,), dtype=torch.float64, device='cuda')),
                dict(scratch=torch.zeros((64,), dtype=torch.float32, device='cuda'))):
        kw = dict(d=d, A=3, g=g, n=n, rec=rec, mask=0b001, scratch=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            episode_stats(r, kw['d'], kw['A'], kw['g'], kw['n'], kw['rec'], side_mask=kw['mask'],
                          scratch=kw['scratch'])
    # more agents than the kernel takes: the bare call is refused, EpisodeStats runs the restatement
    for A9 in (MAX_AGENTS + 1, 40):
        r9, d9, G9, ln9 = _inputs(CH + 1, (5, A9), 'p50', 'half')
        with pytest.raises(ValueError):
            episode_stats(torch.from_numpy(r9).cuda(), torch.from_numpy(d9).cuda(), A9, torch.from_numpy(G9).cuda(),
                          torch.from_numpy(ln9).cuda(), torch.zeros(6 + 2 * A9, dtype=torch.float64, device='cuda'))
        es = EpisodeStats(5, A9, 'cuda', side_mask=0b10101)
        es.ret_carry.copy_(torch.from_numpy(G9))
        es.len_carry.copy_(torch.from_numpy(ln9))
        es.update(torch.from_numpy(r9).cuda().view(CH + 1, 5, A9), torch.from_numpy(d9).cuda())
        want = _restate(CH + 1, (5, A9), 0b10101, 'p50', 'half')
        assert es.ret_carry.cpu().tolist() == want[0].tolist() and es.len_carry.cpu().tolist() == want[1].tolist()
        assert es.last.cpu().tolist() == want[2].tolist() and es.last[0] > 0 and torch.equal(es.total, es.last)
    assert {c[0] for c in CASES} == set(TS) and {c[1] for c in CASES} >= set(EAS) | {BIG}
    assert {c[3] for c in CASES} == set(PATTERNS)
    assert {c[1][1] for c in CASES} == set(range(1, 9))  # every instantiation of the template
    kinds = {('none' if c[2] == 0 else 'full' if c[2] == (1 << c[1][1]) - 1 else
              'lower' if c[2] == (1 << (c[1][1] // 2)) - 1 else 'inter') for c in CASES}
    assert kinds == set(MASKS)
    assert (BIG[0] + WG - 1) // WG > 256
    print('worst |d| / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))
