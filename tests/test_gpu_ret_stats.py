"""mas_ret_stats against the restatement (masurvival.ppo.ret_stats_reference,
held to fp64 by tests/test_reward_norm_reference.py) at the shapes where its
index arithmetic can break: the edges of the 8-step prefetch chunk, the
256-column workgroup edge with envs that straddle it, more than 256 workgroups
(the second pass of k_gae_sums), done flags placed on purpose.  The recurrence
is serial per column, so the carry out has one order and is held bit for bit;
the fp64 sums are held to n 2^-53 sum|term| of the exact sums of the
restatement's returns."""
import numpy as np
import pytest

import ret_ref as R

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import abi  # noqa: E402
from masurvival.ppo import ret_stats, ret_stats_reference  # noqa: E402

F32 = np.float32
SENT, SENT_D = 12345.678, -7.25e300   # what the kernel must leave alone
TS = (1, 7, 8, 9, 16, 17, 64, 65)
COLS = ((1, 1), (21, 3), (85, 3), (64, 4), (257, 1), (86, 3))
PATTERNS = ('none', 'all', 'first', 'last', 'p05', 'p50', 'bytes')
GAMMAS = (0.99, 1.0, 0.0, 0.999)
BIG = (9, (21846, 3))  # 65538 columns: 257 workgroups
WORST = {}


def _cases():
    out = []
    for i in range(3 * len(TS)):
        out.append((TS[i % len(TS)], COLS[(5 * i) % len(COLS)], PATTERNS[i % len(PATTERNS)], GAMMAS[i % len(GAMMAS)]))
    # envs that straddle the 256-column edge at both chunk edges, and the many-workgroup case
    out += [(8, (86, 3), 'p50', 0.99), (65, (86, 3), 'bytes', 0.99), (17, (257, 1), 'last', 0.99),
            BIG + ('p05', 0.99)]
    return out


CASES = _cases()


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


def _inputs(T, E, A, pattern, seed):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((T, E * A)).astype(F32)
    carry = (3.0 * rng.standard_normal(E * A)).astype(F32)   # non-zero going in
    return r, _dones(pattern, T, E, rng), carry


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64 if t.dtype == torch.float64
                               else torch.uint8)


def _run(r, d, carry, gamma, A):
    """mas_ret_stats twice from the same carry, on interior views of larger
    sentinel-filled tensors and with different scratch contents: (carry out,
    sums) as numpy, after the checks that hold for every case."""
    T, M = r.shape
    tr, td = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    keep = [x.clone() for x in (tr, td)]
    n_scr = abi.load_library().mas_ret_stats_scratch_doubles(M)
    assert n_scr == 2 * ((M + 255) // 256)
    outs = []
    for fill in (SENT_D, 3.5e11):
        carry_big = torch.full((M + 8,), SENT, device='cuda')
        carry_big[4:4 + M].copy_(torch.from_numpy(carry))
        sums_big = torch.full((4,), SENT_D, device='cuda', dtype=torch.float64)
        scratch = torch.full((n_scr + 16,), fill, device='cuda', dtype=torch.float64)
        ret_stats(tr, td, gamma, carry_big[4:4 + M], sums_big[1:3], A, scratch=scratch)
        torch.cuda.synchronize()
        assert bool((carry_big[:4] == SENT).all()) and bool((carry_big[4 + M:] == SENT).all()), 'carry overrun'
        assert sums_big[0] == SENT_D and sums_big[3] == SENT_D
        assert bool((scratch[n_scr:] == fill).all()), 'scratch written past mas_ret_stats_scratch_doubles'
        outs.append((carry_big[4:4 + M].clone(), sums_big[1:3].clone()))
    for x, k in zip((tr, td), keep):
        assert torch.equal(_bits(x), _bits(k)), 'an input changed'
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b)), 'two calls with different scratch contents differ'
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()


def _restate(r, d, carry, gamma, A):
    steps = torch.empty(r.shape, dtype=torch.float32)
    new, sums = ret_stats_reference(torch.from_numpy(r), torch.from_numpy(d), gamma, torch.from_numpy(carry), A,
                                    steps_out=steps)
    return steps.numpy(), new.numpy(), sums.numpy()


@pytest.mark.parametrize('T,cols,pattern,gamma', CASES,
                         ids=[f'T{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}' for c in CASES])
def test_carry_bitwise_and_sums_within_the_bound(T, cols, pattern, gamma):
    (E, A), gamma = cols, float(F32(gamma))
    r, d, carry = _inputs(T, E, A, pattern, seed=1000 * T + E)
    got_carry, got_sums = _run(r, d, carry, gamma, A)
    steps, want_carry, ref_sums = _restate(r, d, carry, gamma, A)
    bad = np.argwhere(got_carry.view(np.int32) != want_carry.view(np.int32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    s = R.check_sums(got_sums, steps)
    print(f'sums {s[0]:.3f} {s[1]:.3f} of the bound')
    WORST['sums'] = max(WORST.get('sums', 0.0), *s)
    assert max(s) <= 1.0, (s, got_sums, ref_sums)
    # the restatement itself within its fp64 bound on this case
    assert R.check_steps(r, d, gamma, carry, A, steps) <= 1.0


def test_two_rollouts_chain_through_the_carry():
    """Rows [0, 9) then [9, 26) from the first call's carry: the carry of one
    call over all 26 rows bit for bit, and sums that add up."""
    E, A, gamma = 86, 3, float(F32(0.99))
    r, d, carry = _inputs(26, E, A, 'p05', seed=5)
    c_all, s_all = _run(r, d, carry, gamma, A)
    c_a, s_a = _run(r[:9].copy(), d[:9].copy(), carry, gamma, A)
    c_b, s_b = _run(r[9:].copy(), d[9:].copy(), c_a, gamma, A)
    assert np.array_equal(c_b.view(np.int32), c_all.view(np.int32))
    steps, _, _ = _restate(r, d, carry, gamma, A)
    _, s2, sa = R.exact_sums(steps)
    n = steps.size
    # each of the three within n 2^-53 sum|term| of exact (the parts' n and terms add up), and the addition here
    assert abs(s_a[0] + s_b[0] - s_all[0]) <= (2 * n + 1) * 2.0 ** -53 * sa
    assert abs(s_a[1] + s_b[1] - s_all[1]) <= (2 * n + 1) * 2.0 ** -53 * s2


def test_wrapper_refusals_and_the_case_table():
    r = torch.zeros((4, 6), device='cuda')
    d = torch.zeros((4, 2), dtype=torch.uint8, device='cuda')
    c = torch.zeros((6,), device='cuda')
    s = torch.zeros((2,), dtype=torch.float64, device='cuda')
    ret_stats(r, d, 0.99, c, s, 3)
    torch.cuda.synchronize()
    assert s.tolist() == [0.0, 0.0] and not c.any()
    for bad in (dict(carry=c[:5]), dict(carry=c.double()), dict(sums=s.float()), dict(dones=d.float()),
                dict(n_agents=2), dict(scratch=torch.zeros((1,), dtype=torch.float64, device='cuda'))):
        kw = dict(carry=c, sums=s, dones=d, n_agents=3, scratch=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            ret_stats(r, kw['dones'], 0.99, kw['carry'], kw['sums'], kw['n_agents'], scratch=kw['scratch'])
    assert {c[0] for c in CASES} == set(TS) and {c[1] for c in CASES} == set(COLS) | {BIG[1]}
    assert {c[2] for c in CASES} == set(PATTERNS)
    assert (BIG[1][0] * BIG[1][1] + 255) // 256 == 257
    print('worst |d| / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))
