"""An fp64 restatement of the rollout/update seam (include/masurvival.h
mas_gae, mas_adv_normalize, and the masked statistics of
PPOTrainer.finish_rollout), per-element checkers with derived bounds, and an
fp32 emulation of both kernel forms that the checker's own test mutates.

The formulas, on rewards r [T][M], values V [T + 1][M], done d [T][E] (any
nonzero byte is done; column m belongs to env m // n_agents, E = M / n_agents)
and gamma, lambda already rounded to fp32 (the C ABI takes floats):

  n_t     = 0 where d_t != 0, else 1
  delta_t = r_t + gamma V_{t+1} n_t - V_t
  A_t     = delta_t + c_t A_{t+1},   c_t = gamma lambda n_t,   A_T = 0
  ret_t   = A_t + V_t

gae_ref evaluates this in numpy float64 (the product gamma lambda exact);
test_gae_reference.py pins masurvival.ppo.gae_reference to it on fp64 tensors.

The bound of gae_bound.  With C_{t,s} = prod_{t <= j < s} c_j, A_t = sum_{s >=
t} C_{t,s} delta_s, and with m_s = |r_s| + gamma n_s |V_{s+1}| + |V_s| every
partial sum either kernel forms is at most S_t = sum_{s >= t} C_{t,s} m_s in
magnitude.  The fp32 roundings (each relative u = 2^-24, round to nearest, no
contraction: -ffp-contract=off), to first order in u, as the number k(s - t)
of roundings term s passes through before it reaches A_t:

  delta_s  fl(fl(r + fl(gamma V) n) - V): three roundings, each of a quantity
           of magnitude at most m_s (the product by n is exact): 3.
  walk     (k_gae_walk) per step a = fl(delta + fl(fl(fl(gamma lambda) n) a')):
           the coefficient carries the rounding of the fp32 product gamma lambda
           (the product by n exact), the product c a' rounds, the sum rounds.
           Term s is in the sum at its own step (1) and at each of the s - t
           later ones, where it also passes one coefficient and one product:
           k_walk = 3 + 1 + 3 (s - t) = 4 + 3 (s - t).
  scan     (k_gae) lane q of a 64-step chunk starts with (delta_q, fl(gamma
           lambda) n_q); six Kogge-Stone rounds a = fl(a + fl(b a2)), b = fl(b
           b2) and the carry step A = fl(a + fl(b carry)).
           Sums: a term sits in some lane's a in every round and in the carry
           step, at most 7 roundings of a sum that contains it.
           Coefficient and products inside the chunk: term s reaches lane t by
           one hop per set bit of j = s - t; the b it meets are tree products
           of j raw coefficients in all (j roundings of gamma lambda) joined by
           j - popcount(j) products, and each hop is one product: 2 j.
           Across a chunk boundary at t0 (t < t0 <= s): A_{t0} already carries
           k(s - t0); b spans t0 - t steps (2 (t0 - t) - 1 roundings at most),
           the product with the carry 1, the sum 1: 2 (t0 - t) + 1 more.
           k_scan = 3 + 7 + 2 (s - t) + (boundaries crossed) <= 10 + 3 (s - t),
           since crossing a boundary needs s - t >= 1 per boundary.

ONE bound covers both forms: k(j) = 10 + 3 j (the walk's 4 + 3 j is below it),

  |A_t - fl A_t| <= e_t = u sum_{s >= t} C_{t,s} (10 + 3 (s - t)) m_s,

evaluated as a backward recurrence beside the reference:

  S_t = m_t + c_t S_{t+1},   e_t = 10 u m_t + c_t (e_{t+1} + 3 u S_{t+1}).

ret = fl(A + V) adds one rounding of the stored value: e_t + u |ret_t|.
Nothing here is tuned; a ratio above 1 means a rounding this count misses, or
an error in the kernel.

The sums.  k_gae / k_gae_walk / k_gae_sums add the stored fp32 advantages and
their squares in double, in a fixed tree order.  Each square of an fp32 number
is exact in double, so both are fp64 sums of n exact terms: any order is
within n 2^-53 sum|a| and n 2^-53 sum a^2 of the exact sums (check_sums, the
exact sums by math.fsum).

The normalisation (adv_norm_ref), on the statistics triple (s, q, n) AS GIVEN
(it never recomputes the moments from the data):

  mean = s / n,  var = max(q / n - mean^2, 0)                    (fp64)
  out  = (adv - fl32(mean)) / (fl32(sqrt(var)) + 1e-8f)          (fp32)

adv_norm_ref evaluates `out` in float64 from the two fp32-rounded scalars and
the float constant.  Its bound counts, per element: the rounding of the mean
(u |mean|, should the kernel's double differ from numpy's in the last place
and flip the cast) and the subtraction (u |adv - mean|), both divided by sd;
the square root's cast (u), the addition of 1e-8f (u) and the division (u),
each relative to |out|:  u |mean| / sd + 4 u |out|.
adv_norm_sensitivity gives the first-order change of `out` for statistics
that are off by (ds, dq): the composed bound of the trainer test.

gae_emulate is the kernels' arithmetic in numpy float32 with the named
mutations of MUTATIONS, each an error the checker's test requires to be
caught.  ROUNDING_LEVEL lists the one mutation the bound must accept: gamma
lambda applied without the rounding of its fp32 product.  It moves results by
an ulp or so, within the bound by construction; the exact case (exact_case:
gamma = lambda = 1/2, integers, segments of at most 8 steps, so every
intermediate value of both forms is an fp32 number in any association order)
is held bit for bit and tells it from the kernel exactly where it changes a
bit -- with gamma lambda = 1/4 exact it changes none.
"""
import math

import numpy as np

U = 2.0 ** -24
K0, K1 = 10.0, 3.0      # k(j) = K0 + K1 j (module docstring)
SCAN_COLS = 64          # columns per workgroup of k_gae; its time chunk is 64 steps too
WALK_COLS = 256         # columns per workgroup of k_gae_walk
WALK_CHUNK = 8          # steps the walk prefetches at once
FORMS = ('walk', 'scan')

# name -> the forms it applies to
MUTATIONS = {
    'done_by_column': FORMS,            # done[t][m] instead of done[t][m // n_agents]
    'done_of_next_step': FORMS,         # done[t + 1] used at step t
    'bootstrap_row_T_minus_1': FORMS,   # values[T] read as values[T - 1]
    'delta_not_masked': FORMS,          # the trace masked, delta's gamma V_{t+1} not
    'trace_not_masked': FORMS,          # delta masked, the trace not
    'carry_dropped': ('scan',),         # the carry between scan chunks left at 0
    'carry_from_last_lane': ('scan',),  # the carry read from lane 63, not lane 0
    'walk_tail_skipped': ('walk',),     # the steps after the last whole 8-step chunk
    'ret_next_value': FORMS,            # ret = A + V_{t+1}
    'last_block_unwritten': FORMS,      # the last partial workgroup's columns not stored
    'sums_past_M': FORMS,               # the columns past M of the last workgroup in the sums
    'lambda_on_delta': FORMS,           # A = lambda delta + ...
    'gl_unrounded': FORMS,              # gamma lambda without its fp32 rounding
}
ROUNDING_LEVEL = ('gl_unrounded',)


def _f32_scalars(gamma, lam):
    g, l = np.float32(gamma), np.float32(lam)
    assert float(g) == float(gamma) and float(l) == float(lam), 'pass gamma and lambda already rounded to fp32'
    return g, l


def _not_done(dones, n_agents):
    """n [T][M] float64: 0 where the column's env is done (any nonzero byte)."""
    d = np.asarray(dones)
    return np.repeat((d.reshape(d.shape[0], -1) == 0).astype(np.float64), n_agents, axis=1)


def gae_ref_and_bound(rewards, values, dones, gamma, lam, n_agents):
    """(adv, ret, bound of adv, bound of ret), float64 [T][M] each."""
    g, l = _f32_scalars(gamma, lam)
    g, l = float(g), float(l)
    r = np.asarray(rewards, dtype=np.float64)
    T = r.shape[0]
    r = r.reshape(T, -1)
    v = np.asarray(values, dtype=np.float64).reshape(T + 1, -1)
    n = _not_done(dones, n_agents)
    assert v.shape[1] == r.shape[1] == n.shape[1] and n.shape[0] == T, (r.shape, v.shape, n.shape)
    adv, err = np.empty_like(r), np.empty_like(r)
    a = np.zeros_like(r[0])
    S = np.zeros_like(a)
    e = np.zeros_like(a)
    for t in range(T - 1, -1, -1):
        c = g * l * n[t]
        a = (r[t] + g * v[t + 1] * n[t] - v[t]) + c * a
        m = np.abs(r[t]) + g * n[t] * np.abs(v[t + 1]) + np.abs(v[t])
        e = K0 * U * m + c * (e + K1 * U * S)
        S = m + c * S
        adv[t], err[t] = a, e
    ret = adv + v[:T]
    return adv, ret, err, err + U * np.abs(ret)


def gae_ref(rewards, values, dones, gamma, lam, n_agents):
    """(adv, ret) float64 [T][M] of the module docstring's formulas."""
    return gae_ref_and_bound(rewards, values, dones, gamma, lam, n_agents)[:2]


def gae_bound(rewards, values, dones, gamma, lam, n_agents):
    """(bound of adv, bound of ret) float64 [T][M], absolute, for either form."""
    return gae_ref_and_bound(rewards, values, dones, gamma, lam, n_agents)[2:]


def worst_ratio(got, ref, bound):
    """(worst |got - ref| / bound, its flat position); a non-finite `got` is
    infinitely wrong, d = 0 = bound counts as 0."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    d = np.abs(got - ref)
    q = np.where(d == 0.0, 0.0, d / np.maximum(bound, 1e-300))
    q = np.where(np.isfinite(got), q, np.inf)
    k = int(np.argmax(q))
    return float(q.reshape(-1)[k]), k


def check_gae(rewards, values, dones, gamma, lam, n_agents, adv, ret):
    """Worst |got - ref| / bound of the two outputs against gae_ref of the
    inputs: {'adv': .., 'ret': .., 'at': (t, m) of the worst element}."""
    ra, rr, ba, br = gae_ref_and_bound(rewards, values, dones, gamma, lam, n_agents)
    qa, ka = worst_ratio(adv, ra, ba)
    qr, kr = worst_ratio(ret, rr, br)
    k = ka if qa >= qr else kr
    return {'adv': qa, 'ret': qr, 'at': (k // ra.shape[1], k % ra.shape[1])}


def check_sums(sums, adv_stored):
    """(ratio of sums[0], ratio of sums[1]) against the exact sums of the
    stored fp32 advantages and of their squares, bound n 2^-53 sum|a| (sum a^2)."""
    assert np.asarray(adv_stored).dtype == np.float32
    a = np.asarray(adv_stored, dtype=np.float64).reshape(-1)
    n = a.size
    s1, s2 = math.fsum(a), math.fsum(a * a)  # (a * a exact: 48 bits)
    b1, b2 = n * 2.0 ** -53 * math.fsum(np.abs(a)), n * 2.0 ** -53 * s2
    out = []
    for got, ref, b in ((float(sums[0]), s1, b1), (float(sums[1]), s2, b2)):
        d = abs(got - ref)
        out.append(0.0 if d == 0.0 else (d / max(b, 1e-300) if math.isfinite(got) else math.inf))
    return tuple(out)


def _norm_scalars(stats):
    s, q, n = (float(x) for x in stats)
    mean = s / n
    var = max(q / n - mean * mean, 0.0)
    m32 = np.float32(mean)
    sd32 = np.float32(math.sqrt(var)) + np.float32(1e-8)  # (an fp32 sum)
    assert sd32.dtype == np.float32
    return mean, var, float(m32), float(sd32)


def adv_norm_ref(adv, stats):
    """(adv - fl32(mean)) / (fl32(sqrt(var)) + 1e-8f) in float64, mean and
    var from stats = (sum, sum of squares, count) in float64."""
    _, _, m, sd = _norm_scalars(stats)
    return (np.asarray(adv, dtype=np.float64) - m) / sd


def adv_norm_bound(adv, stats):
    """Per-element absolute bound of the fp32 result (module docstring)."""
    _, _, m, sd = _norm_scalars(stats)
    return U * abs(m) / sd + 4.0 * U * np.abs(adv_norm_ref(adv, stats))


def adv_norm_sensitivity(adv, stats, d_adv, d_s, d_q):
    """First-order bound on the change of adv_norm_ref when adv is off by at
    most d_adv (per element) and the first two statistics by d_s, d_q:
    |d mean| = d_s / n, |d var| = d_q / n + 2 |mean| d_s / n,
    |d sd| = |d var| / (2 sqrt(var)) (var > 0),
    |d out| = (d_adv + |d mean|) / sd + |out| |d sd| / sd."""
    mean, var, _, sd = _norm_scalars(stats)
    n = float(stats[2])
    dm = d_s / n
    dv = d_q / n + 2.0 * abs(mean) * d_s / n
    dsd = dv / (2.0 * math.sqrt(var)) if var > 0.0 else 0.0
    return (np.asarray(d_adv, dtype=np.float64) + dm) / sd + np.abs(adv_norm_ref(adv, stats)) * dsd / sd


def masked_stats_ref(adv, active):
    """(sum w a, sum w a^2, max(sum w, 1)) in float64 (exactly summed, then
    rounded once) for w in {0, 1}."""
    a = np.asarray(adv, dtype=np.float64).reshape(-1)
    w = np.asarray(active, dtype=np.float64).reshape(-1)
    assert a.shape == w.shape and np.all((w == 0.0) | (w == 1.0))
    a = a[w == 1.0]
    return math.fsum(a), math.fsum(a * a), max(float(a.size), 1.0)


def exact_case(T, n_envs, n_agents, seed):
    """(rewards [T][M], values [T + 1][M] float32 integers in [-8, 8], dones
    [T][E] uint8) with a done every 8 steps of each env at a random phase (so
    no segment is longer than 8 steps) and a few more at random; for gamma =
    lambda = 0.5 every intermediate of both kernel forms is exact in fp32."""
    rng = np.random.default_rng(seed)
    M = n_envs * n_agents
    r = rng.integers(-8, 9, size=(T, M)).astype(np.float32)
    v = rng.integers(-8, 9, size=(T + 1, M)).astype(np.float32)
    phase = rng.integers(0, 8, size=n_envs)
    d = ((np.arange(T)[:, None] + phase[None, :]) % 8 == 7) | (rng.random((T, n_envs)) < 0.05)
    return r, v, d.astype(np.uint8)


def _flat_pad(x, n):
    """x flattened, followed by zeros up to n elements (what a read past a
    row lands on: the next row; past the array: taken as zeros)."""
    x = np.asarray(x).reshape(-1)
    return np.concatenate([x, np.zeros(max(n - x.size, 0), dtype=x.dtype)])


def gae_emulate(form, rewards, values, dones, gamma, lam, n_agents, mut=None):
    """(adv, ret) float32 [T][M] and sums (float64 pair) as k_gae_walk
    ('walk') or k_gae ('scan') compute them, every operation in fp32 in the
    kernel's order.  Elements the (mutated) kernel never stores are NaN.
    mut: one of MUTATIONS that applies to the form."""
    assert form in FORMS, form
    assert mut is None or form in MUTATIONS[mut], (form, mut)
    f32 = np.float32
    g, l = _f32_scalars(gamma, lam)
    r = np.asarray(rewards, dtype=f32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    M = r.shape[1]
    A = int(n_agents)
    E = M // A
    v = np.asarray(values, dtype=f32).reshape(T + 1, M)
    d = np.asarray(dones, dtype=np.uint8).reshape(T, E)
    cols = WALK_COLS if form == 'walk' else SCAN_COLS
    Mp = M
    if mut == 'sums_past_M':
        # the last workgroup's lanes past M run too: their reads land on the
        # next row (zeros past the arrays), they store nothing
        Mp = -(-M // cols) * cols
        idx = np.arange(Mp)
        r = np.stack([_flat_pad(rewards, (T + 1) * Mp).astype(f32)[t * M + idx] for t in range(T)])
        v = np.stack([_flat_pad(values, (T + 2) * Mp).astype(f32)[t * M + idx] for t in range(T + 1)])
        dflat = _flat_pad(d, (T + 1) * Mp)
        dcol = np.stack([dflat[t * E + idx // A] for t in range(T)])
    elif mut == 'done_by_column':
        dflat = _flat_pad(d, (T + 1) * M)
        dcol = np.stack([dflat[t * E + np.arange(M)] for t in range(T)])
    else:
        dcol = np.repeat(d, A, axis=1)
    if mut == 'done_of_next_step':
        dcol = np.concatenate([dcol[1:], np.zeros_like(dcol[:1])])
    nt = np.where(dcol != 0, f32(0.0), f32(1.0)).astype(f32)
    nt_delta = np.ones_like(nt) if mut == 'delta_not_masked' else nt
    nt_trace = np.ones_like(nt) if mut == 'trace_not_masked' else nt
    vnext = v[1:].copy()
    if mut == 'bootstrap_row_T_minus_1':
        vnext[T - 1] = v[T - 1]
    delta = (r + (g * vnext) * nt_delta) - v[:T]  # three fp32 roundings, in this order
    if mut == 'lambda_on_delta':
        delta = l * delta
    assert delta.dtype == f32
    # the trace coefficient per step: fl(gamma lambda) n in fp32 (the product by n exact)
    coef = (g * l) * nt_trace
    assert coef.dtype == f32
    if mut == 'gl_unrounded':
        # gamma lambda exact (float64): the first product it enters rounds once, from the exact coefficient
        coef = np.float64(g) * np.float64(l) * nt_trace.astype(np.float64)
    mul = lambda x, y: (x * y).astype(f32)  # noqa: E731  (fp32 operands: the plain fp32 product)

    adv = np.full((T, Mp), np.nan, dtype=f32)
    if form == 'walk':
        a = np.zeros(Mp, dtype=f32)
        t_stop = (T % WALK_CHUNK) if mut == 'walk_tail_skipped' else 0
        for t in range(T - 1, t_stop - 1, -1):
            a = delta[t] + mul(coef[t], a)
            adv[t] = a
    else:
        carry = np.zeros(Mp, dtype=f32)
        for t_hi in range(T, 0, -64):
            t_lo = max(t_hi - 64, 0)
            n = t_hi - t_lo
            a = np.zeros((64, Mp), dtype=f32)   # lanes past the chunk: the identity map
            b = np.ones((64, Mp), dtype=coef.dtype)
            a[:n] = delta[t_lo:t_hi]
            b[:n] = coef[t_lo:t_hi]
            off = 1
            while off < 64:  # Kogge-Stone, suffix order: lane q takes lane q + off's map after its own
                a2, b2 = a[off:].copy(), b[off:].copy()
                a[:64 - off] = a[:64 - off] + mul(b[:64 - off], a2)
                b[:64 - off] = mul(b[:64 - off], b2)
                off *= 2
            At = a + mul(b, carry)
            assert At.dtype == f32
            if mut != 'carry_dropped':
                carry = At[63] if mut == 'carry_from_last_lane' else At[0]
            adv[t_lo:t_hi] = At[:n]
    assert adv.dtype == f32
    ret = adv + (vnext if mut == 'ret_next_value' else v[:T])
    fin = np.where(np.isnan(adv), 0.0, adv.astype(np.float64))
    sums = (float(np.sum(fin)), float(np.sum(fin * fin)))
    adv, ret = adv[:, :M].copy(), ret[:, :M].copy()
    if mut == 'last_block_unwritten' and M % cols:
        adv[:, M - M % cols:] = np.nan
        ret[:, M - M % cols:] = np.nan
    return adv, ret, sums
