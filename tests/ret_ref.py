"""An fp64 restatement of the running discounted returns behind the reward
normalisation (include/masurvival.h mas_ret_stats), a per-step checker with a
derived bound, and an fp32 emulation that the checker's own test mutates.

The formulas, on rewards r [T][M], done d [T][E] (any nonzero byte is done;
column m belongs to env m // n_agents, E = M / n_agents), the carry R_{-1} [M]
and gamma already rounded to fp32 (the C ABI takes a float).  Step t does, in
this order,

  R_t = gamma R_{t-1} + r_t            (R_{t-1} taken as 0 after a done step)
  the step counts: sums += (R_t, R_t^2)
  a done step resets what the NEXT step sees, not what this one counted.

ret_ref evaluates it in numpy float64 from the fp32 carry as given.

The bound.  The kernel computes fl(fl(gamma R) + r): two fp32 roundings (each
relative u = 2^-24, round to nearest, no contraction).  With
S_t = |gamma| S_{t-1} + |r_t|, S_{-1} = |carry|, every value either rounding
sees at step t is at most S_t in magnitude (the product at most |gamma|
S_{t-1}), to first order in u.  The error e_{t-1} of R_{t-1} passes through the
product (|gamma| e_{t-1}), the product rounds (u |gamma| S_{t-1}), the sum
rounds (u S_t):

  e_t = |gamma| (e_{t-1} + u S_{t-1}) + u S_t,   e_{-1} = 0,

and S and e are zeroed after a done step as R is.  Nothing here is tuned; a
ratio above 1 means a rounding this count misses, or an error in the code
under test.

The sums.  R is an fp32 number, so R and R^2 are exact in double and the
kernel's sums are fp64 sums of n = T M exact terms in a fixed tree order: any
order is within n 2^-53 sum|R| and n 2^-53 sum R^2 of the exact sums
(check_sums, the exact sums by math.fsum).

ret_emulate is the kernel's arithmetic in numpy float32 with the named
mutations of MUTATIONS, each an error the checker's test requires to be caught.
"""
import math

import numpy as np

U = 2.0 ** -24
COLS = 256   # columns per workgroup of k_ret_stats
CHUNK = 8    # steps it prefetches at once

MUTATIONS = (
    'reset_before_counting',   # a done step counts 0 instead of its return
    'done_by_column',          # done[t][m] instead of done[t][m // n_agents]
    'carry_ignored',           # every column starts from 0
    'gamma_on_reward',         # R = gamma (R + r)
)


def _f32_gamma(gamma):
    g = np.float32(gamma)
    assert float(g) == float(gamma), 'pass gamma already rounded to fp32'
    return g


def _done_cols(dones, n_agents):
    """[T][M] bool: the column's env is done (any nonzero byte)."""
    d = np.asarray(dones)
    return np.repeat(d.reshape(d.shape[0], -1) != 0, n_agents, axis=1)


def ret_ref_and_bound(rewards, dones, gamma, carry, n_agents):
    """(R float64 [T][M] as every step counted it, its absolute bound [T][M],
    the carry out float64 [M])."""
    g = float(_f32_gamma(gamma))
    r = np.asarray(rewards, dtype=np.float64)
    T = r.shape[0]
    r = r.reshape(T, -1)
    d = _done_cols(dones, n_agents)
    assert np.asarray(carry).dtype == np.float32, 'the carry is the fp32 state as stored'
    R = np.asarray(carry, dtype=np.float64).reshape(-1).copy()
    assert d.shape == r.shape and R.shape == r[0].shape, (r.shape, d.shape, R.shape)
    S = np.abs(R)
    e = np.zeros_like(R)
    out, err = np.empty_like(r), np.empty_like(r)
    for t in range(T):
        R = g * R + r[t]
        S_new = abs(g) * S + np.abs(r[t])
        e = abs(g) * (e + U * S) + U * S_new
        S = S_new
        out[t], err[t] = R, e
        R = np.where(d[t], 0.0, R)
        S = np.where(d[t], 0.0, S)
        e = np.where(d[t], 0.0, e)
    return out, err, R


def ret_ref(rewards, dones, gamma, carry, n_agents):
    return ret_ref_and_bound(rewards, dones, gamma, carry, n_agents)[0]


def worst_ratio(got, ref, bound):
    """(worst |got - ref| / bound, its flat position); a non-finite `got` is
    infinitely wrong, d = 0 = bound counts as 0."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    d = np.abs(got - ref)
    q = np.where(d == 0.0, 0.0, d / np.maximum(bound, 1e-300))
    q = np.where(np.isfinite(got), q, np.inf)
    k = int(np.argmax(q))
    return float(q.reshape(-1)[k]), k


def check_steps(rewards, dones, gamma, carry, n_agents, steps):
    """Worst |steps - ref| / bound of the per-step returns [T][M]."""
    ref, bound, _ = ret_ref_and_bound(rewards, dones, gamma, carry, n_agents)
    return worst_ratio(steps, ref, bound)[0]


def exact_sums(steps):
    """(sum R, sum R^2, sum |R|) of stored fp32 returns, each summed exactly
    and rounded once."""
    assert np.asarray(steps).dtype == np.float32
    a = np.asarray(steps, dtype=np.float64).reshape(-1)
    return math.fsum(a), math.fsum(a * a), math.fsum(np.abs(a))  # (a * a exact: 48 bits)


def check_sums(sums, steps):
    """(ratio of sums[0], ratio of sums[1]) against the exact sums of the
    fp32 returns `steps` and of their squares, bound n 2^-53 sum|R| (sum R^2)."""
    s1, s2, sa = exact_sums(steps)
    n = np.asarray(steps).size
    out = []
    for got, ref, b in ((float(sums[0]), s1, n * 2.0 ** -53 * sa), (float(sums[1]), s2, n * 2.0 ** -53 * s2)):
        d = abs(got - ref)
        out.append(0.0 if d == 0.0 else (d / max(b, 1e-300) if math.isfinite(got) else math.inf))
    return tuple(out)


def moments(steps_list):
    """(count, mean, m2) in float64, two passes, of all the per-step returns in
    the list of arrays."""
    x = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in steps_list])
    mean = math.fsum(x) / x.size
    return float(x.size), mean, math.fsum((x - mean) ** 2)


def check_state(state, steps_list):
    """state (count, mean, m2) against the two-pass fp64 moments of all merged
    returns.  The sums are within n 2^-53 sum|term| of exact (check_sums) and
    m2 comes from sum R^2 - n mean^2 plus a few fp64 roundings per merge, each
    far below one of those: 8 n 2^-52 sum|term| for both, as the observation
    normaliser's trainer test builds it."""
    n, mean, m2 = moments(steps_list)
    x = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in steps_list])
    got = np.asarray(state, dtype=np.float64)
    assert got[0] == n, (got[0], n)
    tol = 8 * n * 2.0 ** -52
    assert abs(got[1] - mean) <= tol * math.fsum(np.abs(x)) / n + 1e-300, (got[1], mean)
    assert abs(got[2] - m2) <= tol * math.fsum(x * x) + 1e-300, (got[2], m2)


def scale_of(state, eps):
    """fl32(1 / sqrt(m2 / count + eps)) of a (count, mean, m2) state."""
    return np.float32(1.0 / math.sqrt(float(state[2]) / float(state[0]) + eps))


def ret_emulate(rewards, dones, gamma, carry, n_agents, mut=None):
    """(R float32 [T][M] as counted, the carry out float32 [M], sums (float64
    pair)) as k_ret_stats computes them, every operation in fp32 in the
    kernel's order.  mut: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS, mut
    f32 = np.float32
    g = _f32_gamma(gamma)
    r = np.asarray(rewards, dtype=f32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    M = r.shape[1]
    d = np.asarray(dones, dtype=np.uint8).reshape(T, -1)
    if mut == 'done_by_column':
        flat = np.concatenate([d.reshape(-1), np.zeros((T + 1) * M, dtype=np.uint8)])
        dcol = np.stack([flat[t * d.shape[1] + np.arange(M)] for t in range(T)]) != 0
    else:
        dcol = np.repeat(d != 0, n_agents, axis=1)
    R = np.asarray(carry, dtype=f32).reshape(-1).copy()
    if mut == 'carry_ignored':
        R = np.zeros_like(R)
    out = np.empty((T, M), dtype=f32)
    for t in range(T):
        if mut == 'gamma_on_reward':
            R = g * (R + r[t])
        else:
            R = (g * R) + r[t]   # two fp32 roundings, in this order
        assert R.dtype == f32
        if mut == 'reset_before_counting':
            R = np.where(dcol[t], f32(0.0), R)
        out[t] = R
        R = np.where(dcol[t], f32(0.0), R)
    o64 = out.astype(np.float64)
    return out, R, (float(np.sum(o64)), float(np.sum(o64 * o64)))
