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

The six parameter gradients a minibatch ends with (check_grads) are sums over
the rows of the stored tensors, so they are teacher-forced as well:

  dW1 = dA1_k^T x, db1 = sum dA1_k;  dW2 = dA2_k^T h1_k, db2 = sum dA2_k;
  dW3 = dz_k^T h2_k, db3 = sum dz_k  (where h2 and dz were stored; the fused
  kernel's layer 3 stays with check_dw3)

in fp64.  Nothing is rounded to bf16 on the way where the sum is an fp32 one
(mas_policy_dw, the in-kernel dW3): FP32 (|a|^T |h|) + 1e-6 per element, the
bound of test_policy_dw_matches_fp32.  The split-K GEMMs of masurvival.ppo
(_splitk_nn for layer 1, _splitk_nt, _splitk_tn) are torch.bmm on bf16
operands: each K-chunk's partial product S_c is rounded to bf16 before the
fp32 sum over the chunks, half a bf16 ulp of each, so such a gradient carries
BF16_HALF_ULP sum_c |S_c| on top, S_c the fp64 partial products of the chunks
ppo._split_k(M) makes; their bias columns (the product with the ones column)
the same with S_c = the chunk's column sums.  That term is the larger one by
far: a GEMM gradient is 10 to 65 times the fp32 bound off (check_grads reports
the figure as '<tensor>_x_fp32').

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


def loss_rows(z, acts, old_logp, adv, ret, clip, vf_coef, ent_coef, scale, row_w=None):
    """The per-row PPO loss and its gradient at z [M, 16] fp64, stated head by
    head from the formula of include/masurvival.h (no autograd):
      row i, head hd, output k:  scale (g_i (1[k = a_hd] - p_k) + ent_coef p_k (log p_k + H_hd)),
      g_i = -ratio adv where ratio adv <= clip(ratio) adv, else 0;
      value: scale vf_coef 2 (v - ret).
    row_w [M] (mas_policy_train_w): row i's g_i and entropy term times w_i, the
    value term as it is; 'w' of the result is that weight (ones without)."""
    dt = torch.float64
    z, old_logp, adv, ret = z.to(dt), old_logp.to(dt), adv.to(dt), ret.to(dt)
    w = torch.ones_like(adv) if row_w is None else row_w.to(dt)
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
        dz[:, off:off + n] = scale * w[:, None] * (g[:, None] * (onehot - p) + ent_coef * p * (lsm + H[:, None]))
    dv = z[:, 15] - ret
    dz[:, 15] = scale * vf_coef * 2.0 * dv
    return dict(dz=dz, ratio=ratio, s1=s1, pg=-torch.minimum(s1, s2), vl=dv * dv, ent=ent, w=w,
                clipped=((ratio - 1.0).abs() > clip).to(dt))


def _tanh_bound(ref, abs_pre, c):
    return BF16_HALF_ULP * ref.abs() + c * (1.0 - ref * ref) * abs_pre + TANH_ABS


def _logit_err(P, h2, c):
    return c * (h2.abs() @ P['W3'].abs().T + P['b3'].abs()).max(1).values + 1e-6


def _dz_bound(L, d, cf):
    clip, vf, ec, sc = cf
    pol = L['w'][:, None] * (8.0 * L['s1'].abs()[:, None] + 4.0 * ec)  # the weighted terms (w = 1 without row_w)
    return BF16_HALF_ULP * L['dz'].abs() + sc * d[:, None] * (pol + 2.0 * vf)


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


def check_dw3(P, x, batch, cf, gw, gb, c=FP32, row_w=None, h2k=None):
    """Worst |d| / bound of the layer-3 gradients gw [16, 256], gb [16] against
    dz^T h2 and the column sums of dz of the unforced fp64 chain; the bound is
    the per-row bounds of check_rows summed over the rows (module docstring).
    row_w: the rows' weights of mas_policy_train_dw3_w (loss_rows).
    Returns {'dw3': .., 'db3': ..}.

    h2k: the h2 [M, 256] a train kernel stored for these rows and this packed
    policy (the unfused kernel's, whose data path is the fused one's): the
    check is then teacher-forced on it, as check_rows is -- logits h2k W3^T +
    b3, no h2 term in the bound.  That is what rows of a real rollout need:
    the surrogate's gradient jumps at a clip boundary, and the bf16 rounding of
    h1 and h2 moves a log-ratio by about 1e-3, so among a rollout's rows some
    fall on the other side of a boundary in the unforced chain than in the
    kernel, each by its whole surrogate term, which no rounding bound covers
    (make_batch keeps its rows 0.01 away instead).  Forced, the kernel's ratio
    is within 12 d_i of the reference's (six heads, each log-prob within twice
    the logit error d_i); a row whose reference ratio is that close to the
    boundary that counts for its advantage's sign may still fall on either
    side, and the bound grants exactly those rows ('flip_rows' of the result)
    their surrogate term."""
    acts, old_logp, adv, ret = batch
    clip, vf, ec, sc = cf
    if h2k is None:
        h1, h2, z = forward(P, x)
    else:
        h2 = h2k.double()
        z = h2 @ P['W3'].T + P['b3']
    L = loss_rows(z, acts, old_logp, adv, ret, clip, vf, ec, sc, row_w)
    dz = L['dz']
    d = _logit_err(P, h2, c)
    bdz = _dz_bound(L, d, cf)
    res = {}
    if h2k is None:
        bh2 = _tanh_bound(h2, h1.abs() @ P['W2'].abs().T + P['b2'].abs(), c)
        bw = bdz.T @ h2.abs() + dz.abs().T @ bh2 + c * (dz.abs().T @ h2.abs()) + 1e-6
    else:
        a = adv.double()
        # s1 <= s2: ratio <= 1 + clip (adv > 0), ratio >= 1 - clip (adv < 0)
        edge = torch.where(a > 0, 1.0 + clip, 1.0 - clip)
        flip = (a != 0) & ((L['ratio'] - edge).abs() <= 12.0 * d * L['ratio'])
        on = loss_rows(z, acts, old_logp, adv, ret, 1e30, vf, ec, sc, row_w)['dz']                     # never clipped
        off = loss_rows(z, acts, old_logp, torch.zeros_like(adv), ret, clip, vf, ec, sc, row_w)['dz']  # no surrogate
        bdz = bdz + flip[:, None] * (on - off).abs()
        bw = bdz.T @ h2.abs() + c * (dz.abs().T @ h2.abs()) + 1e-6
        res['flip_rows'] = int(flip.sum())
    bb = bdz.sum(0) + c * dz.abs().sum(0) + 1e-6
    res.update(dw3=_worst(gw.double() - dz.T @ h2, bw), db3=_worst(gb.double() - dz.sum(0), bb))
    return res


GRADS = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')


def _check_layer(a, h, gw, gb, gemm, chunks, c):
    """Worst |d| / bound of gw [F, G] against a^T h and of gb [F] against the
    column sums of a (a [M, F], h [M, G], fp64); gemm: the bound carries the
    bf16 rounding of the `chunks` partial products.  Returns (w, b, w over the
    fp32-only bound, b over it)."""
    M = a.shape[0]
    dw, db = gw.double() - a.T @ h, gb.double() - a.sum(0)
    bw = c * (a.abs().T @ h.abs()) + 1e-6
    bb = c * a.abs().sum(0) + 1e-6
    xw, xb = _worst(dw, bw), _worst(db, bb)
    if not gemm:
        return xw, xb, xw, xb
    assert M % chunks == 0, (M, chunks)
    ac, hc = a.reshape(chunks, M // chunks, -1), h.reshape(chunks, M // chunks, -1)
    bw = bw + BF16_HALF_ULP * torch.bmm(ac.transpose(1, 2), hc).abs().sum(0)
    bb = bb + BF16_HALF_ULP * ac.sum(1).abs().sum(0)
    return _worst(dw, bw), _worst(db, bb), xw, xb


def check_grads(x, out, grads, gemm=(1,), chunks=1, c=FP32):
    """Worst |d| / bound of the parameter gradients `grads` (dict w1 [256, D],
    b1, w2 [256, 256], b2 [256], w3 [16, 256], b3 [16]) against the fp64 sums
    over the rows of the kernel's own stored tensors: x [M, D + 1] with the ones
    column, and `out` with h1, da1, da2 and, where they were stored, h2 and dz
    [M, F] in natural order (without them layer 3 is left out).  gemm: the
    layers (1, 2, 3) whose gradient went through a bf16-output split-K GEMM of
    `chunks` = ppo._split_k(M) chunks; the others are fp32 sums (module
    docstring).  Returns {tensor: worst ratio} and, for the GEMM layers,
    '<tensor>_x_fp32': the same error over the fp32-only bound."""
    d = lambda t: t.double()  # noqa: E731
    x = d(x)
    D = x.shape[1] - 1
    assert bool((x[:, D] == 1.0).all()), 'x: column D must be the ones column'
    layers = [(1, d(out['da1']), x[:, :D]), (2, d(out['da2']), d(out['h1']))]
    if 'h2' in out and 'dz' in out:
        layers.append((3, d(out['dz']), d(out['h2'])))
    res = {}
    for n, a, h in layers:
        wk, bk = f'w{n}', f'b{n}'
        assert grads[wk].shape == (a.shape[1], h.shape[1]) and grads[bk].shape == (a.shape[1],), (wk, grads[wk].shape)
        res[wk], res[bk], xw, xb = _check_layer(a, h, grads[wk], grads[bk], n in gemm, chunks, c)
        if n in gemm:
            res[wk + '_x_fp32'], res[bk + '_x_fp32'] = xw, xb
    return res


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


# ---------------------------------------------------------------------------
# The gradient assembly of FusedPolicy.grads on the host, from the stored
# tensors of emulate(): fp32 sums (mas_policy_dw, the in-kernel dW3: any row
# order) or the bf16-output split-K GEMMs of masurvival.ppo, with the named
# assembly errors the checker's test requires check_grads to reject.

# name -> the tensors that must reject it
GRAD_MUTATIONS = {
    'last_row_dropped': GRADS, 'row_counted_twice': GRADS,
    'db_from_neighbour': ('b1', 'b2'), 'dw2_transposed': ('w2',), 'dw2_from_h2': ('w2',),
    'dw1_bias_from_column_D-1': ('b1',), 'scale_1_over_M_missing': GRADS,
    'rm_permutation_not_undone': ('w1', 'b1', 'w2', 'b2', 'w3'),
}


def stand_in_permutation():
    """A feature -> stored column permutation of the 256 hidden features that
    stays inside the 32-feature tiles, as the row-major kernel's does
    (mas_policy_rm_feature; the host test has no library to ask)."""
    g = torch.Generator().manual_seed(32)
    return torch.cat([32 * t + torch.randperm(32, generator=g) for t in range(8)])


def emulate_grads(x, out, mode='fp32', mut=None, gen=None):
    """{w1 .. b3} from x [M, D + 1] (ones column included) and emulate()'s out.
    mode 'fp32': fp32 matmuls over the rows in a shuffled order (gen);
    'gemm': layer 1 through ppo._splitk_nn, layers 2 and 3 through
    ppo._splitk_nt, on bf16 operands with the ones row, as FusedPolicy.grads
    has them where mas_policy_dw does not apply."""
    from masurvival import ppo
    M, D = x.shape[0], x.shape[1] - 1
    rows = torch.randperm(M, generator=gen) if mode == 'fp32' else torch.arange(M)
    if mut == 'last_row_dropped':
        rows = rows[rows != M - 1]
    if mut == 'row_counted_twice':
        rows = torch.cat([rows, torch.tensor([1 % M])])
    T = {k: out[k].float()[rows] for k in ('h1', 'h2', 'da1', 'da2', 'dz')}
    T['h2w'] = T['h2']
    if mut == 'rm_permutation_not_undone':  # the stored column order kept where a feature index is meant
        q = stand_in_permutation()
        inv = torch.empty_like(q)
        inv[q] = torch.arange(256)
        T = {k: (v if k == 'dz' else v[:, inv]) for k, v in T.items()}
    x = x.float()[rows]
    ones = torch.ones((x.shape[0], 1))
    pairs = {1: (T['da1'], x), 2: (T['da2'], torch.cat([T['h2' if mut == 'dw2_from_h2' else 'h1'], ones], 1)),
             3: (T['dz'], torch.cat([T['h2w'], ones], 1))}
    g = {}
    for n, (a, h) in pairs.items():
        if mode == 'fp32':
            full = a.T @ h
        elif n == 1:
            full = ppo._splitk_nn(a.T.bfloat16(), h.bfloat16())
        else:
            full = ppo._splitk_nt(a.T.bfloat16(), h.T.bfloat16())
        G = h.shape[1] - 1
        g[f'w{n}'], g[f'b{n}'] = full[:, :G].clone(), full[:, G].clone()
        if n == 1 and mut == 'dw1_bias_from_column_D-1':
            g['b1'] = full[:, D - 1].clone()
    if mut == 'dw2_transposed':
        g['w2'] = g['w2'].T.clone()
    if mut == 'db_from_neighbour':
        g['b1'], g['b2'] = g['b2'], g['b1']
    if mut == 'scale_1_over_M_missing':
        g = {k: v * M for k, v in g.items()}
    return g
