"""A host restatement of the action sampler (include/masurvival.h
mas_sample_actions; k_sample in csrc/mas_capi.hip, act_sample_split and the
one-half loop of k_policy_act in csrc/mas_policy.hip) and a per-row checker of
what those kernels draw.  numpy only.

The stream (all of it uint64 arithmetic that wraps):

  mix64(z): SplitMix64's output function, z += 0x9E3779B97F4A7C15 first
  base(seed, step, row) = mix64(seed ^ mix64(step * 0x100000001B3 + row))
  r(h, k) = mix64(base + 4 h + k)           head h in [0, 6), option k in [0, n_h)
  u = ((float)(r >> 40) + 0.5f) * 2^-24     in fp32

row is the row's index in the whole batch (first_row + the row of the call).
x = r >> 40 < 2^24 converts exactly; x + 0.5 is exact only for x < 2^23, above
it rounds to even, so u lies in (0, 1]: x = 0 gives 2^-25, x = 2^24 - 1 gives
1.0.  The score of option k is g = z_k - log(-log(u)) and the head's action the
first option with the greatest score (a strict > scan from option 0).  u = 1.0
gives -log(u) = -0, log(-0) = -inf and g = +inf: the option wins whatever the
logits, with a finite log-prob.

The checker (check_draws) forms the scores in fp64 from the fp32 logits the
caller supplies and the fp32 u.  A head whose best two fp64 scores are closer
than tau may go either way in the kernels' fp32; any other head must draw the
reference's option.

tau is derived, not measured: an fp32 score has magnitude at most max(|z|,
17.33) (17.33 = -log(2^-25), and |log(-log u)| <= 17.33 for every u < 1), and
the operations behind one score -- one add, two hardware logs at 1 ulp, two
multiplies by ln 2 -- account for fewer than 8 ulps.  tau is 64 ulps at that
magnitude: 2^-13 while max |z| < 32, doubling with each binade above.

The log-prob bound is derived the same way, 8 2^-24 sum_h (|z_chosen| + |lse_h|
+ 1), against the fp64 log-softmax of the same logits at the kernel's own
actions.

Two scores made of the same (z, u) are equal in any precision: such an exact
tie is decided (the lower index wins), not near."""
import numpy as np

HEAD_N = (3, 3, 3, 2, 2, 2)
HEAD_OFF = (0, 3, 6, 9, 11, 13)
N_LOGITS = 15
X_MAX = (1 << 24) - 1   # r >> 40 of the draw with u = 1.0
U_MIN = 2.0 ** -25      # u of r >> 40 = 0
NEAR_CAP = 0.005        # the share of rows with a near-tie head every case stays under

_U = np.uint64
_GOLDEN = _U(0x9E3779B97F4A7C15)
_M1 = _U(0xBF58476D1CE4E5B9)
_M2 = _U(0x94D049BB133111EB)
_STEP_MUL = _U(0x100000001B3)
_MASK32 = (1 << 32) - 1

# deliberate errors of the stream or the scan (sample(mut=...)); the checker's
# test requires check_draws to reject each
MUTATIONS = ('head_dropped', 'heads_2_4_swapped', 'row_mod_32', 'first_row_dropped', 'step_lo32', 'seed_lo32',
             'u_low_bits', 'scan_ge', 'third_logit_zero')


def _u64(v):
    return np.asarray(v if not isinstance(v, int) else v & ((1 << 64) - 1), dtype=np.uint64)


def mix64(z):
    z = _u64(z)
    with np.errstate(over='ignore'):
        z = z + _GOLDEN
        z = (z ^ (z >> _U(30))) * _M1
        z = (z ^ (z >> _U(27))) * _M2
    return z ^ (z >> _U(31))


def base(seed, step, row):
    """row: the index in the whole batch (int or array)."""
    with np.errstate(over='ignore'):
        return mix64(_u64(seed) ^ mix64(_u64(step) * _STEP_MUL + _u64(row)))


def draws(b):
    """r(h, k) for bases b [M] -> uint64 [M, 6, 3] (k = 2 of a two-option head
    is a draw no kernel makes)."""
    key = (4 * np.arange(6, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :])
    with np.errstate(over='ignore'):
        return mix64(np.atleast_1d(_u64(b))[:, None, None] + key[None])


def u_from_x(x):
    """u of x = r >> 40 as the kernels form it, in np.float32."""
    x = np.asarray(x).astype(np.float32)
    return (x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def u_from_r(r):
    return u_from_x(_u64(r) >> _U(40))


def _rows(rows):
    if isinstance(rows, (int, np.integer)):
        return np.arange(int(rows), dtype=np.uint64)
    return np.asarray(rows).astype(np.uint64)


def stream_u(seed, step, first_row, rows, mut=None):
    """fp32 u [M, 6, 3] of rows (a count, or the rows' indices in the call)."""
    rows = _rows(rows)
    if mut == 'row_mod_32':
        rows = rows % _U(32)
    if mut == 'first_row_dropped':
        first_row = 0
    if mut == 'step_lo32':
        step = step & _MASK32
    if mut == 'seed_lo32':
        seed = seed & _MASK32
    with np.errstate(over='ignore'):
        b = base(seed, step, _u64(first_row) + rows)
    r = draws(b)
    if mut == 'head_dropped':
        r = np.repeat(r[:, :1], 6, axis=1)
    if mut == 'heads_2_4_swapped':
        r = r[:, [0, 1, 4, 3, 2, 5]]
    if mut == 'u_low_bits':
        return u_from_x(r & _U(X_MAX))
    return u_from_r(r)


def scores(logits, u, third=-np.inf):
    """fp64 scores [M, 6, 3] of fp32 logits [M, >= 15] and fp32 u [M, 6, 3];
    the third option of a two-option head scores -inf (`third`: the logit a
    mutation reads there).  Also returns the logits as [M, 6, 3] fp64."""
    lg = np.asarray(logits)
    assert lg.dtype == np.float32 and u.dtype == np.float32
    M = lg.shape[0]
    z = np.full((M, 6, 3), -np.inf)
    for h, (n, off) in enumerate(zip(HEAD_N, HEAD_OFF)):
        z[:, h, :n] = lg[:, off:off + n]
        if n < 3:
            z[:, h, n:] = third
    with np.errstate(divide='ignore'):
        g = z - np.log(-np.log(u.astype(np.float64)))
    return g, z


def choose(g, ge=False):
    """The scan from option 0: strict > keeps the first of equal scores (ge:
    the mutated scan, which keeps the last)."""
    if ge:
        return (2 - np.argmax(g[..., ::-1], axis=-1)).astype(np.int8)
    return np.argmax(g, axis=-1).astype(np.int8)


def sample(logits, seed, step, first_row, rows, mut=None):
    """The reference's actions int8 [M, 6] (mut: one of MUTATIONS)."""
    u = stream_u(seed, step, first_row, rows, mut)
    g, _ = scores(logits, u, third=0.0 if mut == 'third_logit_zero' else -np.inf)
    return choose(g, ge=mut == 'scan_ge')


def tau(z):
    """The near-tie threshold per row and head [M, 6] of logits z [M, 6, 3]."""
    zm = np.where(np.isfinite(z), np.abs(z), 0.0).max(-1)
    e = np.floor(np.log2(np.maximum(zm, 1.0)))
    return 2.0 ** (-13.0 + np.maximum(e - 4.0, 0.0))


def top2(g, z, u):
    """(best, second, margin) per row and head: the scan's choice, the
    runner-up (the scan's choice among the rest) and the gap of their scores;
    inf where the two are made of the same (z, u) -- equal in any precision, the
    lower index wins -- or where only the best is infinite."""
    best = choose(g).astype(np.int64)
    g2 = g.copy()
    np.put_along_axis(g2, best[..., None], -np.inf, -1)
    second = np.argmax(g2, axis=-1)
    pick = lambda a, i: np.take_along_axis(a, i[..., None], -1)[..., 0]  # noqa: E731
    gb, gs = pick(g, best), pick(g, second)
    with np.errstate(invalid='ignore'):
        margin = gb - gs
    same = (pick(z, best) == pick(z, second)) & (pick(u, best) == pick(u, second))
    margin = np.where(np.isnan(margin), 0.0, margin)
    margin = np.where(same, np.inf, margin)
    return best, second, margin


def log_prob(logits, acts):
    """(fp64 log-prob [M] of acts [M, 6], the derived bound [M]) from the fp64
    log-softmax of fp32 logits.  An action outside its head counts as option 0
    here (check_draws reports it under 'range')."""
    lg = np.asarray(logits).astype(np.float64)
    acts = np.asarray(acts).astype(np.int64)
    M = lg.shape[0]
    lp, mag = np.zeros(M), np.zeros(M)
    for h, (n, off) in enumerate(zip(HEAD_N, HEAD_OFF)):
        zz = lg[:, off:off + n]
        mx = zz.max(1)
        lse = mx + np.log(np.exp(zz - mx[:, None]).sum(1))
        a = np.where((acts[:, h] >= 0) & (acts[:, h] < n), acts[:, h], 0)
        zc = np.take_along_axis(zz, a[:, None], 1)[:, 0]
        lp += zc - lse
        mag += np.abs(zc) + np.abs(lse) + 1.0
    return lp, 8.0 * 2.0 ** -24 * mag


def check_draws(logits, seed, step, first_row, rows, acts, logp):
    """The kernel's acts int8 [M, 6] and logp fp32 [M] of rows (a count, or the
    rows' indices in the call; first_row + row keys the stream) on fp32 logits
    [M, >= 15], against the restatement.  Returns
      wrong         heads with margin >= tau whose action is not the reference's
      outside_top2  heads with margin < tau whose action is neither of the top two
      near_share    the share of rows with any head under tau
      range         actions outside [0, n_h)
      logp          worst |logp - ref| / bound (inf for a non-finite logp)
    and, for the record: 'near_heads', 'runner_up' (heads that drew the
    runner-up) and 'runner_up_margin' (the largest margin among them, 0 if none)."""
    lg = np.ascontiguousarray(np.asarray(logits)[:, :N_LOGITS])
    acts = np.asarray(acts).astype(np.int64)
    logp = np.asarray(logp).astype(np.float64)
    u = stream_u(seed, step, first_row, rows)
    assert lg.shape[0] == u.shape[0] == acts.shape[0] == logp.shape[0]
    g, z = scores(lg, u)
    best, second, margin = top2(g, z, u)
    near = margin < tau(z)
    is_best, is_second = acts == best, acts == second
    n = np.asarray(HEAD_N)[None, :]
    ref, bound = log_prob(lg, acts)
    with np.errstate(invalid='ignore'):
        ratio = np.abs(logp - ref) / bound
    ratio = np.where(np.isfinite(logp), ratio, np.inf)
    ru = is_second & ~is_best
    return {
        'wrong': int((~near & ~is_best).sum()),
        'outside_top2': int((near & ~is_best & ~is_second).sum()),
        'near_share': float(near.any(1).mean()),
        'range': int(((acts < 0) | (acts >= n)).sum()),
        'logp': float(ratio.max()),
        'near_heads': int(near.sum()),
        'runner_up': int(ru.sum()),
        'runner_up_margin': float(margin[ru].max()) if ru.any() else 0.0,
    }


def near_share(logits, seed, step, first_row=0):
    """The reference alone: the share of rows with any head under tau."""
    lg = np.ascontiguousarray(np.asarray(logits)[:, :N_LOGITS])
    u = stream_u(seed, step, first_row, lg.shape[0])
    g, z = scores(lg, u)
    return float((top2(g, z, u)[2] < tau(z)).any(1).mean())


# ---------------------------------------------------------------------------
# Extreme draws.  EXTREME holds what search_extreme found, as (seed, step, row,
# head, option): 'one' has r >> 40 = 2^24 - 1 (u = 1.0), 'min' has r >> 40 = 0
# (u = 2^-25), 'tie' has equal r >> 40 at options `option` and `option + 1`, the
# greatest of its head (on equal logits an exact tie of the two best scores).  'fused': any row, reached
# through first_row; 'sample': row < 4096 (mas_sample_actions has no
# first_row), found over step.

SEARCH_SEED = 20261
SEARCH_CHUNK = 1 << 20


def search_extreme(seed, step0, n_steps, row0, n_rows, want=('one', 'min', 'tie')):
    """The first tuple of each kind in `want`, over steps [step0, step0 +
    n_steps) and rows [row0, row0 + n_rows), in chunks; stops when all are found."""
    found = {}
    valid = np.zeros((6, 3), dtype=bool)
    for h, n in enumerate(HEAD_N):
        valid[h, :n] = True
    for step in range(step0, step0 + n_steps):
        for lo in range(row0, row0 + n_rows, SEARCH_CHUNK):
            rows = np.arange(lo, min(lo + SEARCH_CHUNK, row0 + n_rows), dtype=np.uint64)
            x = draws(base(seed, step, rows)) >> _U(40)
            hits = {'one': (x == _U(X_MAX)) & valid, 'min': (x == _U(0)) & valid}
            t = np.zeros(x.shape, dtype=bool)
            top = np.where(valid[None], x, _U(0)).max(-1, keepdims=True)
            t[:, :, :2] = (x[:, :, :2] == x[:, :, 1:]) & valid[None, :, 1:] & (x[:, :, :2] == top)
            hits['tie'] = t
            for kind in want:
                if kind not in found and hits[kind].any():
                    i, h, k = (int(v[0]) for v in np.nonzero(hits[kind]))
                    found[kind] = (seed, step, int(rows[i]), h, k)
            if len(found) == len(want):
                return found
    return found


def search_all():
    """What EXTREME was made from (a few seconds each)."""
    return {'fused': search_extreme(SEARCH_SEED, 11, 1, 1 << 35, 1 << 25),
            'sample': search_extreme(SEARCH_SEED, 0, 1 << 13, 0, 4096)}


EXTREME = {
    'fused': {'one': (20261, 11, 34361793480, 5, 1), 'min': (20261, 11, 34360055654, 0, 2),
              'tie': (20261, 11, 34368823405, 5, 0)},
    'sample': {'one': (20261, 21, 3378, 0, 1), 'min': (20261, 139, 910, 0, 1), 'tie': (20261, 1748, 507, 5, 0)},
}


def extreme_x(t):
    """r >> 40 of every option of the tuple's head: uint64 [3]."""
    seed, step, row, h, _ = t
    return draws(base(seed, step, row))[0, h] >> _U(40)
