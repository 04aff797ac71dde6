"""An fp64 restatement of the PPO optimizer step (include/masurvival.h
mas_policy_adam: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam,
no weight decay, no amsgrad), a per-element checker with a derived bound, and
an fp32 emulation of the kernel's arithmetic that the checker's own test
mutates.

The step, on the fp32 inputs p, g, m, v [n] and the Python-double scalars:

  g'   = grad_scale g
  coef = min(1, max_norm / (|g'|_2 + 1e-6))        (max_norm <= 0: 1, no clip)
  gc   = coef g'
  m'   = m + (1 - beta1) (gc - m)                  (exp_avg.lerp_)
  v'   = beta2 v + (1 - beta2) gc^2                (mul_, addcmul_)
  den  = sqrt(v') / sqrt(1 - beta2^step) + eps
  p'   = p - (lr / (1 - beta1^step)) m' / den      (addcdiv_)

adam_ref evaluates this in numpy float64; test_update_reference.py pins it to
torch.optim.Adam + clip_grad_norm_ on fp64 tensors (1e-12 relative).

The bound of check_adam counts the fp32 roundings of k_adam_update
(csrc/mas_policy.hip; no contraction: -ffp-contract=off; division and square
root correctly rounded), each relative u = 2^-24, to first order in u:

  scalars  step_size = fl(lr / bc1), sqrt_bc2 = fl(sqrt(bc2)), w1 = fl(1 - beta1),
           w2 = fl(1 - beta2), b2 = fl(beta2), eps = fl(eps): u each.
  coef     the fp32 sum of squares is within FP32 (the project's fp32
           dot-product constant, relative for a sum of non-negative terms) of
           |g'|^2; the square root halves that and rounds (u), + 1e-6f (u, the
           float constant included), the division (u):
           EC = FP32 / 2 + 4 u, and only where coef < 1: fminf(.., 1) is exact.
  gc       fl(fl(g scale) coef): relative EG = EC + 2 u.
  m'       fl(m + fl(w1 fl(gc - m))): the subtraction, w1 and the product,
           3 u |w1 (gc - m)|; the input error w1 |gc| EG; the last addition is
           the rounding of the stored value, u |m'|:
           em = w1 |gc| EG + 3 u w1 |gc - m| + u |m'|.
  v'       fl(fl(v b2) + fl(w2 fl(gc gc))): gc^2 carries 2 EG + u, w2 and its
           product 2 u; b2 and its product 2 u; the stored value u |v'|:
           ev = w2 gc^2 (2 EG + 3 u) + 2 u beta2 v + u v'.
  den      fl(fl(fl(sqrt(v')) / sqrt_bc2) + eps): the square root halves v''s
           relative error and rounds, esq = sqrt(v') (ev / (2 v') + u) (0 at
           v' = 0); sqrt_bc2 and the division 2 u; eps u; the addition u:
           eden = esq / sqrt_bc2 + 2 u sqrt(v') / sqrt_bc2 + u eps + u den.
  p'       r = fl(m' / den): er = em / den + |r| eden / den + u |r|;
           t = fl(step_size r): et = step_size er + 2 u |t|;
           p' = fl(p + t), the stored value: ep = et + u |p'|.

Nothing here is tuned; a ratio above 1 means a rounding this count misses, or
an error in the kernel.

adam_emulate is the kernel's arithmetic in numpy float32 with the named
mutations of MUTATIONS, each an error the checker's test requires to be caught.
"""
import math

import numpy as np

U = 2.0 ** -24
FP32 = 1e-5  # policy_rows_ref.FP32: fp32 dot-product error per unit of sum |a| |b|
BLOCK = 256             # threads of a k_adam_update block (one element each per pass)
FIRST_PASS = 512 * 256  # elements of the first grid-stride pass: min(ceil(n / 256), 512) blocks

MUTATIONS = ('w2_from_float_beta', 'no_bias_correction2', 'eps_inside_sqrt', 'coef_without_1e-6',
             'norm_of_unscaled_grad', 'tail_skipped', 'second_pass_skipped')


def _terms(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step):
    """The fp64 step with its intermediate values (module docstring)."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    p, g, m, v = f(p), f(g), f(m), f(v)
    b1, b2 = float(betas[0]), float(betas[1])
    gs = g * float(grad_scale)
    coef = 1.0
    if max_norm > 0.0:
        coef = min(1.0, float(max_norm) / (math.sqrt(float(np.sum(gs * gs))) + 1e-6))
    gc = gs * coef
    w1, w2 = 1.0 - b1, 1.0 - b2
    m1 = m + w1 * (gc - m)
    v1 = b2 * v + w2 * gc * gc
    sbc2 = math.sqrt(1.0 - b2 ** step)
    step_size = float(lr) / (1.0 - b1 ** step)
    sq = np.sqrt(v1)
    den = sq / sbc2 + float(eps)
    r = m1 / den
    p1 = p - step_size * r
    return dict(p=p, m=m, v=v, gc=gc, coef=coef, w1=w1, w2=w2, b2=b2, m1=m1, v1=v1, sbc2=sbc2, step_size=step_size,
                sq=sq, den=den, r=r, p1=p1, eps=float(eps))


def adam_ref(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step):
    """(p', m', v') in float64 of one clip + Adam step on the fp32 (or fp64)
    inputs; `step` is the step being taken (>= 1)."""
    t = _terms(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step)
    return t['p1'], t['m1'], t['v1']


def adam_bounds(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step):
    """((p', m', v') fp64, (ep, em, ev) the per-element bounds of the module docstring)."""
    t = _terms(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step)
    ec = FP32 / 2.0 + 4.0 * U if t['coef'] < 1.0 else 0.0
    eg = ec + 2.0 * U
    gc, w1, w2 = np.abs(t['gc']), t['w1'], t['w2']
    em = w1 * gc * eg + 3.0 * U * w1 * np.abs(t['gc'] - t['m']) + U * np.abs(t['m1'])
    ev = w2 * gc * gc * (2.0 * eg + 3.0 * U) + 2.0 * U * t['b2'] * t['v'] + U * t['v1']
    pos = t['v1'] > 0.0
    esq = np.where(pos, t['sq'] * (ev / (2.0 * np.where(pos, t['v1'], 1.0)) + U), 0.0)
    eden = esq / t['sbc2'] + 2.0 * U * t['sq'] / t['sbc2'] + U * t['eps'] + U * t['den']
    r = np.abs(t['r'])
    er = em / t['den'] + r * eden / t['den'] + U * r
    et = t['step_size'] * er + 2.0 * U * t['step_size'] * r
    ep = et + U * np.abs(t['p1'])
    return (t['p1'], t['m1'], t['v1']), (ep, em, ev)


def check_adam(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step, p_new, m_new, v_new):
    """Worst |d| / bound of the step's three outputs (any float arrays [n])
    against adam_ref of the inputs: {'p': .., 'm': .., 'v': ..}.  An element
    with d = 0 = bound counts as 0."""
    ref, bounds = adam_bounds(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step)
    res = {}
    for k, new, rf, bd in zip('pmv', (p_new, m_new, v_new), ref, bounds):
        d = np.abs(np.asarray(new, dtype=np.float64) - rf)
        assert d.shape == rf.shape, (k, d.shape, rf.shape)
        res[k] = float(np.max(d / np.maximum(bd, 1e-300)))
    return res


def adam_emulate(p, g, m, v, grad_scale, max_norm, lr, betas, eps, step, mut=None):
    """(p', m', v') float32 as k_adam_sqsum + k_adam_update compute them: the
    launcher's double scalars rounded once to float, every operation in fp32.
    mut: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS, mut
    f32 = np.float32
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    n = p.shape[0]
    b1, b2 = float(betas[0]), float(betas[1])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    step_size, sqrt_bc2 = f32(lr / bc1), f32(math.sqrt(bc2))
    w1, w2, b2f, epsf = f32(1.0 - b1), f32(1.0 - b2), f32(b2), f32(eps)
    if mut == 'w2_from_float_beta':
        w2 = f32(1.0) - f32(b2)
    if mut == 'no_bias_correction2':
        sqrt_bc2 = f32(1.0)
    scale, mx = f32(grad_scale), f32(max_norm)
    gs = g * scale
    x = g if mut == 'norm_of_unscaled_grad' else gs
    s = np.sum(x * x, dtype=f32)
    coef = f32(1.0)
    if mx > 0.0:
        norm = np.sqrt(s) if mut == 'coef_without_1e-6' else np.sqrt(s) + f32(1e-6)
        coef = min(f32(mx / norm), f32(1.0))
    gi = gs * coef
    mi = m + w1 * (gi - m)
    vi = v * b2f + w2 * (gi * gi)
    if mut == 'eps_inside_sqrt':
        den = np.sqrt(vi + epsf) / sqrt_bc2
    else:
        den = np.sqrt(vi) / sqrt_bc2 + epsf
    pi = p + (-step_size) * (mi / den)
    assert pi.dtype == f32 and mi.dtype == f32 and vi.dtype == f32
    keep = np.zeros(n, dtype=bool)  # elements the mutated kernel never visits
    if mut == 'tail_skipped':
        keep[n - n % BLOCK:] = True
    if mut == 'second_pass_skipped':
        keep[FIRST_PASS:] = True
    return np.where(keep, p, pi), np.where(keep, m, mi), np.where(keep, v, vi)
