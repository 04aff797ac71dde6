"""A staged fp64 reference of the PPO train kernels (include/masurvival.h
mas_policy_train*), a per-element checker, and an fp32 + bf16 emulation of the
kernels that the checker's own test mutates.

Every stage is compared teacher-forced: the reference of a stage starts from
the kernel's own stored output of the stage before, so a comparison carries
one stage's error and the bound is about one bf16 rounding:

  h1  = tanh(x W1^T + b1)
  h2  = tanh(h1_k W2^T + b2)
  z   = h2_k W3^T + b3                          (not stored; feeds dz)
  dz  = the PPO loss gradient at z, written out head by head in loss_rows()
  dA2 = (dz_k W3) (1 - h2_k^2)
  dA1 = (dA2_k W2) (1 - h1_k^2)
  partials.sum(0) = sums over the rows of -min(s1, s2), (v - ret)^2, the
                    entropy and [|ratio - 1| > clip]

(_k: as the kernel stored it.)  All reference arithmetic is torch.float64 on
what the kernel reads: the bf16-rounded weight matrices, the fp32 biases (the
packed image keeps them in fp32) and the bf16 x rows.

Bounds, per element: a rounding term 2^-8 |ref| (half a bf16 ulp, relative:
the one rounding of the stored value) plus an fp32 term, FP32 (1e-5, the
constant of test_policy_dw_matches_fp32) times sum |a| |b| over the dot
product that feeds the element; for h1 / h2 times the slope 1 - ref^2, plus
1e-6 absolute for the cancellation in tanh_pre's 1 - 2 / (e + 1) near 0.
dz: with d_i = FP32 max_o (|h2_k| |W3|^T + |b3|) + 1e-6 the logit error of row
i, the fp32 term is scale d_i (8 |ratio adv| + 4 ent_coef + 2 vf_coef) (six
heads' log-probs enter the ratio, plus p itself).  The three summed partials:
FP32 sum |term|; the clipped count: equal.

The layer-3 gradient of the fused kernel (check_dw3) has nothing stored to
force with: dW3 = dz^T h2 and db3 = the column sums of dz from the unforced
fp64 chain, bounded by the per-row bounds summed over the rows,
sum_i (dz bound |h2| + |dz| h2 bound) + FP32 |dz|^T |h2| + 1e-6.  The per-row
terms are the teacher-forced ones: what the bf16 rounding of h1 and h2 does to
the logits further down is not in them.  Those errors are of random sign and
per row smaller than the rounding term, while the bound adds absolute
values over the rows, so it holds for a minibatch (0.04 to 0.14 of it
measured at 512 rows) and not for a single row, where it is not used.

Tensors here are row-major in natural feature order: h1, h2, dA1, dA2
[M, 256], dz [M, 16]; the tests transpose / un-permute what the kernels store.
"""
import torch

HEAD_N = (3, 3, 3, 2, 2, 2)
HEAD_OFF = (0, 3, 6, 9, 11, 13)
N_OUT = 16
FP32 = 1e-5          # fp32 dot-product error per unit of sum |a| |b| (test_policy_dw_matches_fp32)
BF16_HALF_ULP = 2.0 ** -8
TANH_ABS = 1e-6
STAGES = ('h1', 'h2', 'dz', 'da2', 'da1', 'partials')

# coefficient sets (clip, vf_coef, ent_coef, scale * M)
COEF = {'A': (0.2, 0.5, 0.01, 1.0), 'B': (0.1, 1.0, 0.05, 0.5), 'C': (0.2, 0.0, 1.0, 1.0)}
DEFAULT_COEF = COEF['A']


def coef(name, M):
    clip, vf, ec, sm = COEF[name]
    return clip, vf, ec, sm / M


def make_policy(D, kind='plain'):
    """PolicyMLP(D, 256) seeded by D; 'x4': every parameter times 4 (saturated
    tanh, peaked heads); 'zero': times 0 with head.bias = linspace(-1, 1, 16)
    (z is the biases)."""
    torch.manual_seed(D + 1)
    from masurvival.ppo import PolicyMLP
    p = PolicyMLP(D, 256)
    with torch.no_grad():
        s = {'plain': 1.0, 'x4': 4.0, 'zero': 0.0}[kind]
        for q in p.parameters():
            q.mul_(s)
        if kind == 'zero':
            p.head.bias.copy_(torch.linspace(-1.0, 1.0, 16))
    return p


def params(policy):
    """What the packed image holds of a PolicyMLP, as fp64: bf16-rounded weight
    matrices, fp32 biases."""
    ts = [policy.body[0].weight, policy.body[0].bias, policy.body[2].weight, policy.body[2].bias,
          policy.head.weight, policy.head.bias]
    ts = [t.detach().float() for t in ts]
    W1, b1, W2, b2, W3, b3 = ts
    rw = lambda w: w.bfloat16().double()  # noqa: E731
    return dict(W1=rw(W1), b1=b1.double(), W2=rw(W2), b2=b2.double(), W3=rw(W3), b3=b3.double())


def forward(P, x):
    """The unforced fp64 chain: (h1, h2, z) of x [M, D]."""
    x = x.double()
    h1 = torch.tanh(x @ P['W1'].T + P['b1'])
    h2 = torch.tanh(h1 @ P['W2'].T + P['b2'])
    return h1, h2, h2 @ P['W3'].T + P['b3']


def head_log_softmax(z):
    """[(log p [M, n]) per head] of z [M, >= 15]."""
    out = []
    for n, off in zip(HEAD_N, HEAD_OFF):
        zz = z[:, off:off + n]
        out.append(zz - torch.logsumexp(zz, 1, keepdim=True))
    return out


def log_prob(z, acts):
    lp = torch.zeros(z.shape[0], dtype=z.dtype, device=z.device)
    for hd, lsm in enumerate(head_log_softmax(z)):
        lp = lp + lsm.gather(1, acts[:, hd:hd + 1].long()).squeeze(1)
    return lp


def loss_rows(z, acts, old_logp, adv, ret, clip, vf_coef, ent_coef, scale):
    """The per-row PPO loss and its gradient at z [M, 16] fp64, stated head by
    head from the formula of include/masurvival.h (no autograd):
      row i, head hd, output k:  scale (g_i (1[k = a_hd] - p_k) + ent_coef p_k (log p_k + H_hd)),
      g_i = -ratio adv where ratio adv <= clip(ratio) adv, else 0;
      value: scale vf_coef 2 (v - ret)."""
    dt = torch.float64
    z, old_logp, adv, ret = z.to(dt), old_logp.to(dt), adv.to(dt), ret.to(dt)
    lsms = head_log_softmax(z)
    lp = log_prob(z, acts)
    ratio = torch.exp(lp - old_logp)
    s1 = ratio * adv
    s2 = ratio.clamp(1.0 - clip, 1.0 + clip) * adv
    g = torch.where(s1 <= s2, -s1, torch.zeros_like(s1))
    dz = torch.zeros_like(z)
    ent = torch.zeros_like(lp)
    for hd, (n, off, lsm) in enumerate(zip(HEAD_N, HEAD_OFF, lsms)):
        p = lsm.exp()
        H = -(p * lsm).sum(1)
        ent = ent + H
        onehot = (torch.arange(n, device=z.device)[None, :] == acts[:, hd:hd + 1].long()).to(dt)
        dz[:, off:off + n] = scale * (g[:, None] * (onehot - p) + ent_coef * p * (lsm + H[:, None]))
    dv = z[:, 15] - ret
    dz[:, 15] = scale * vf_coef * 2.0 * dv
    return dict(dz=dz, ratio=ratio, s1=s1, pg=-torch.minimum(s1, s2), vl=dv * dv, ent=ent,
                clipped=((ratio - 1.0).abs() > clip).to(dt))


def _tanh_bound(ref, abs_pre, c):
    return BF16_HALF_ULP * ref.abs() + c * (1.0 - ref * ref) * abs_pre + TANH_ABS


def _logit_err(P, h2, c):
    return c * (h2.abs() @ P['W3'].abs().T + P['b3'].abs()).max(1).values + 1e-6


def _dz_bound(L, d, cf):
    clip, vf, ec, sc = cf
    return BF16_HALF_ULP * L['dz'].abs() + sc * d[:, None] * (8.0 * L['s1'].abs()[:, None] + 4.0 * ec + 2.0 * vf)


def _worst(d, bound):
    """max |d| / bound; an element with d = 0 = bound counts as 0."""
    return float((d.abs() / bound.clamp_min(1e-300)).max())


def near_clip_rows(ratio, clip, eps=1e-3):
    """Rows whose ratio is within eps of a clip boundary (the tests need none)."""
    return int((((ratio - (1.0 - clip)).abs() < eps) | ((ratio - (1.0 + clip)).abs() < eps)).sum())


def check_rows(P, x, batch, cf, out, c=FP32):
    """Worst |d| / bound of every stage of `out` (dict h1, h2, dz, da2, da1
    [M, F] and partials [4], any float dtype) against the teacher-forced fp64
    reference.  batch = (acts int8 [M, 6], old_logp, adv, ret); cf = (clip,
    vf_coef, ent_coef, scale).  Returns {stage: worst ratio} for STAGES, plus
    'clipped' (kernel count - reference count) and 'near_clip' (rows of the
    reference ratio within 1e-3 of a clip boundary)."""
    acts, old_logp, adv, ret = batch
    clip, vf, ec, sc = cf
    d = lambda t: t.double()  # noqa: E731
    x = d(x)
    h1k, h2k, dzk, da2k, da1k = (d(out[k]) for k in ('h1', 'h2', 'dz', 'da2', 'da1'))
    W1, b1, W2, b2, W3 = P['W1'], P['b1'], P['W2'], P['b2'], P['W3']
    res = {}
    ref = torch.tanh(x @ W1.T + b1)
    res['h1'] = _worst(h1k - ref, _tanh_bound(ref, x.abs() @ W1.abs().T + b1.abs(), c))
    ref = torch.tanh(h1k @ W2.T + b2)
    res['h2'] = _worst(h2k - ref, _tanh_bound(ref, h1k.abs() @ W2.abs().T + b2.abs(), c))
    L = loss_rows(h2k @ W3.T + P['b3'], acts, old_logp, adv, ret, clip, vf, ec, sc)
    res['dz'] = _worst(dzk - L['dz'], _dz_bound(L, _logit_err(P, h2k, c), cf))
    s2 = 1.0 - h2k * h2k
    ref = (dzk @ W3) * s2
    res['da2'] = _worst(da2k - ref, BF16_HALF_ULP * ref.abs() + c * (dzk.abs() @ W3.abs()) * s2)
    s1 = 1.0 - h1k * h1k
    ref = (da2k @ W2) * s1
    res['da1'] = _worst(da1k - ref, BF16_HALF_ULP * ref.abs() + c * (da2k.abs() @ W2.abs()) * s1)
    part = d(out['partials'])
    sums = torch.stack([L[k].sum() for k in ('pg', 'vl', 'ent')])
    bsum = c * torch.stack([L[k].abs().sum() for k in ('pg', 'vl', 'ent')])
    res['partials'] = _worst(part[:3] - sums, bsum)
    res['clipped'] = float(part[3] - L['clipped'].sum())
    res['near_clip'] = near_clip_rows(L['ratio'], clip)
    return res


def check_dw3(P, x, batch, cf, gw, gb, c=FP32):
    """Worst |d| / bound of the layer-3 gradients gw [16, 256], gb [16] against
    dz^T h2 and the column sums of dz of the unforced fp64 chain; the bound is
    the per-row bounds of check_rows summed over the rows (module docstring).
    Returns {'dw3': .., 'db3': ..}."""
    acts, old_logp, adv, ret = batch
    clip, vf, ec, sc = cf
    h1, h2, z = forward(P, x)
    L = loss_rows(z, acts, old_logp, adv, ret, clip, vf, ec, sc)
    dz = L['dz']
    bdz = _dz_bound(L, _logit_err(P, h2, c), cf)
    bh2 = _tanh_bound(h2, h1.abs() @ P['W2'].abs().T + P['b2'].abs(), c)
    bw = bdz.T @ h2.abs() + dz.abs().T @ bh2 + c * (dz.abs().T @ h2.abs()) + 1e-6
    bb = bdz.sum(0) + c * dz.abs().sum(0) + 1e-6
    return {'dw3': _worst(gw.double() - dz.T @ h2, bw), 'db3': _worst(gb.double() - dz.sum(0), bb)}


def make_batch(P, x, cf, gen, h2=None, zero_adv_every=5):
    """The tests' minibatch for rows x: actions sampled from the reference
    logits; old_logp = lp_ref - log t with t cycling through 0.5, both sides
    of both clip boundaries at 0.01, 0.95, 1, 1.05 and 2 (so ratio_ref = t);
    random advantages, every fifth row exactly 0; ret = v_ref + noise.
    h2: the kernel's stored h2 of these rows (it does not depend on the batch):
    the reference logits are then the teacher-forced ones check_rows compares
    against, h2 W3^T + b3, and every row's reference ratio is exactly its t,
    0.01 or more from a clip boundary whatever the bf16 rounding of h1 and h2
    did to the logits (with 4x weights it moves log-probs by about 0.01).
    gen: a torch.Generator on x's device."""
    from masurvival.ppo import sample_actions
    clip = cf[0]
    z = forward(P, x)[2] if h2 is None else h2.double() @ P['W3'].T + P['b3']
    acts, _ = sample_actions(z[:, :15].float(), gen)
    lp = log_prob(z, acts)
    M, dev = x.shape[0], x.device
    t = torch.tensor([0.5, 1 - clip - 0.01, 1 - clip + 0.01, 0.95, 1.0, 1.05, 1 + clip - 0.01, 1 + clip + 0.01, 2.0],
                     dtype=torch.float64, device=dev)
    rows = torch.arange(M, device=dev)
    old_logp = (lp - t[rows % 9].log()).float()
    adv = torch.randn((M,), device=dev, generator=gen)
    adv[rows % zero_adv_every == 0] = 0.0
    ret = z[:, 15].float() + torch.randn((M,), device=dev, generator=gen)
    return acts.contiguous(), old_logp.contiguous(), adv.contiguous(), ret.contiguous()


# ---------------------------------------------------------------------------
# The emulation: the kernels' arithmetic in fp32 with bf16 rounding at the five
# stored tensors and the exp2-based tanh of tanh_pre.  `mut` names one
# deliberate error (MUTATIONS); the checker's test requires each to be caught.

_LOG2E = 1.4426950408889634
_LN2 = 0.6931471805599453

# name -> the stage that must reject it
MUTATIONS = {
    'entropy_dropped': 'dz', 'entropy_sign': 'dz', 'entropy_total': 'dz', 'entropy_last_head_missing': 'dz',
    'value_factor_2_missing': 'dz', 'clip_ignored': 'dz', 'clip_wrong_side_negative_adv': 'dz',
    'coefs_fixed_at_defaults': 'dz', 'scale_fixed_at_1_over_M': 'dz',
    'dtanh_omitted_da2': 'da2', 'dtanh_from_h1_da2': 'da2', 'w2_not_transposed_da1': 'da1',
    'swap_features_odd_rows_h1': 'h1', 'swap_features_odd_rows_h2': 'h2', 'swap_features_odd_rows_da2': 'da2',
    'swap_features_odd_rows_da1': 'da1',
    'row_shift_h1': 'h1', 'row_shift_h2': 'h2', 'row_shift_dz': 'dz', 'row_shift_da2': 'da2', 'row_shift_da1': 'da1',
}
ENTROPY_MUTATIONS = ('entropy_dropped', 'entropy_sign', 'entropy_total', 'entropy_last_head_missing')


def _bf(t):
    return t.bfloat16().float()


def _tanh_k(a, b):
    c = torch.tensor(2.0 * _LOG2E, dtype=torch.float32, device=a.device)
    e = torch.exp2(a * c + b * c)
    return 1.0 - 2.0 / (e + 1.0)


def _exp_k(x):
    return torch.exp2(x * _LOG2E)


def _loss_k(z, acts, old_logp, adv, ret, cf, mut):
    """The loss gradient as the kernels compute it (fp32, exp2 / log2)."""
    clip, vf, ec, sc = cf
    M = z.shape[0]
    if mut == 'coefs_fixed_at_defaults':
        vf, ec = DEFAULT_COEF[1], DEFAULT_COEF[2]
    if mut == 'scale_fixed_at_1_over_M':
        sc = 1.0 / M
    f32 = torch.float32
    lsms, ps, Hs = [], [], []
    lp = torch.zeros(M, dtype=f32, device=z.device)
    ent = torch.zeros(M, dtype=f32, device=z.device)
    for hd, (n, off) in enumerate(zip(HEAD_N, HEAD_OFF)):
        zz = z[:, off:off + n]
        mx = zz.max(1, keepdim=True).values
        lse = mx + torch.log2(_exp_k(zz - mx).sum(1, keepdim=True)) * _LN2
        lsm = zz - lse
        p = _exp_k(lsm)
        H = -(p * lsm).sum(1)
        lp = lp + lsm.gather(1, acts[:, hd:hd + 1].long()).squeeze(1)
        ent = ent + H
        lsms.append(lsm), ps.append(p), Hs.append(H)
    ratio = _exp_k(lp - old_logp)
    s1 = ratio * adv
    s2 = ratio.clamp(1.0 - clip, 1.0 + clip) * adv
    g = torch.where(s1 <= s2, -s1, torch.zeros_like(s1))
    if mut == 'clip_ignored':
        g = -s1
    if mut == 'clip_wrong_side_negative_adv':  # the positive-advantage rule for every row
        g = torch.where(ratio <= 1.0 + clip, -s1, torch.zeros_like(s1))
    dz = torch.zeros((M, N_OUT), dtype=f32, device=z.device)
    for hd, (n, off) in enumerate(zip(HEAD_N, HEAD_OFF)):
        p, lsm, H = ps[hd], lsms[hd], Hs[hd]
        onehot = (torch.arange(n, device=z.device)[None, :] == acts[:, hd:hd + 1].long()).to(f32)
        e = ec
        if mut == 'entropy_dropped' or (mut == 'entropy_last_head_missing' and hd == 5):
            e = 0.0
        if mut == 'entropy_sign':
            e = -ec
        if mut == 'entropy_total':
            H = ent
        dz[:, off:off + n] = sc * (g[:, None] * (onehot - p) + e * p * (lsm + H[:, None]))
    dv = z[:, 15] - ret
    dz[:, 15] = sc * vf * (1.0 if mut == 'value_factor_2_missing' else 2.0) * dv
    part = torch.stack([(-torch.minimum(s1, s2)).sum(), (dv * dv).sum(), ent.sum(),
                        ((ratio - 1.0).abs() > clip).float().sum()])
    return dz, part


def _store(name, v, mut):
    """The stored image of v [M, F] under a layout mutation of tensor `name`."""
    if mut == 'swap_features_odd_rows_' + name:  # features 3 and 4 of the 32-feature tile 2, odd rows
        v = v.clone()
        a, b = 2 * 32 + 3, 2 * 32 + 4
        v[1::2, a], v[1::2, b] = v[1::2, b].clone(), v[1::2, a].clone()
    if mut == 'row_shift_' + name:  # row r lands in column r + 1
        v = torch.cat([v[:1], v[:-1]], 0)
    return v


def emulate(P, x, batch, cf, mut=None):
    """The kernels' outputs for rows x as `out` of check_rows, plus 'dw3' and
    'db3' (fp32 sums of the bf16 dz and h2, as the fused kernel accumulates)."""
    acts, old_logp, adv, ret = batch
    W1, b1, W2, b2, W3, b3 = (P[k].float() for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'))
    x = x.float()
    h1 = _bf(_tanh_k(x @ W1.T, b1))
    h2 = _bf(_tanh_k(h1 @ W2.T, b2))
    z = h2 @ W3.T + b3
    dz32, part = _loss_k(z, acts, old_logp.float(), adv.float(), ret.float(), cf, mut)
    dz = _bf(dz32)
    g2 = dz @ W3
    if mut == 'dtanh_omitted_da2':
        da2 = _bf(g2)
    elif mut == 'dtanh_from_h1_da2':
        da2 = _bf(g2 * (1.0 - h1 * h1))
    else:
        da2 = _bf(g2 * (1.0 - h2 * h2))
    g1 = da2 @ (W2.T if mut == 'w2_not_transposed_da1' else W2)
    da1 = _bf(g1 * (1.0 - h1 * h1))
    out = {k: _store(k, v, mut) for k, v in (('h1', h1), ('h2', h2), ('dz', dz), ('da2', da2), ('da1', da1))}
    out['partials'] = part
    out['dw3'] = dz.T @ h2
    out['db3'] = dz.sum(0)
    return out
