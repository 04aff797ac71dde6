"""The power of the per-row checker of the PPO train kernels
(tests/policy_rows_ref.py), measured on the CPU: the fp32 + bf16 emulation of
the kernels passes every bound, and each of a list of deliberate errors in the
emulation overshoots the bound of the stage it belongs to at least ten times.
The bounds of test_gpu_policy_rows.py are thereby a checked property: tight
enough that an entropy term with the wrong sign, a dtanh from the wrong tile
or a row stored one column over cannot hide in them."""
import functools

import pytest
import torch

import policy_rows_ref as R

REJECT = 10.0  # a mutation must overshoot its stage's bound at least this many times

# (D, M): the small shapes of the GPU cases
DW3_SHAPE = (160, 512)  # the case of the fused layer-3 gradient check
SHAPES = [(160, 326), (138, 512), (468, 130), (138, 326), (160, 77), (138, 77), (138, 1)]


@functools.lru_cache(maxsize=None)
def _case(D, M, kind, cset):
    P = R.params(R.make_policy(D, kind))
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((M, D), generator=g) * 2.0).bfloat16()
    cf = R.coef(cset, M)
    if (D, M) == DW3_SHAPE:  # the unforced check: the batch from the unforced logits
        return P, x, R.make_batch(P, x, cf, g), cf
    # h2 does not depend on the batch: a first pass on a null batch yields it
    null = (torch.zeros((M, 6), dtype=torch.int8), torch.zeros(M), torch.zeros(M), torch.zeros(M))
    h2 = R.emulate(P, x, null, cf)['h2']
    return P, x, R.make_batch(P, x, cf, g, h2=h2), cf


def _run(D, M, kind, cset, mut=None):
    P, x, batch, cf = _case(D, M, kind, cset)
    out = R.emulate(P, x, batch, cf, mut)
    res = R.check_rows(P, x, batch, cf, out)
    if (D, M) == DW3_SHAPE:
        res.update(R.check_dw3(P, x, batch, cf, out['dw3'], out['db3']))
    return res


CLEAN = ([(D, M, 'plain', 'A') for D, M in SHAPES] + [(160, 326, 'plain', c) for c in 'BC'] +
         [(138, 77, 'plain', c) for c in 'BC'] + [(160, 512, 'plain', c) for c in 'BC'] +
         [(160, 326, 'x4', 'A'), (138, 512, 'x4', 'A'), (160, 326, 'zero', 'A'), (138, 512, 'zero', 'A')])


@pytest.mark.parametrize('D,M,kind,cset', CLEAN)
def test_emulation_passes_the_checker(D, M, kind, cset):
    res = _run(D, M, kind, cset)
    print(D, M, kind, cset, {k: round(v, 3) for k, v in res.items()})
    for k in R.STAGES + (('dw3', 'db3') if (D, M) == DW3_SHAPE else ()):
        assert res[k] <= 1.0, (k, res)
    assert res['clipped'] == 0.0 and res['near_clip'] == 0, res


def test_batch_reaches_both_sides_of_both_clip_boundaries():
    """make_batch, at the smallest many-row shape: within 0.011 of either clip
    boundary, on either side, rows with either sign of the advantage; rows
    with advantage exactly 0; no row nearer than 0.009."""
    for cset in 'AB':
        P, x, (acts, old_logp, adv, ret), cf = _case(138, 77, 'plain', cset)
        clip = cf[0]
        z = R.emulate(P, x, (acts, old_logp, adv, ret), cf)['h2'].double() @ P['W3'].T + P['b3']
        ratio = R.loss_rows(z, acts, old_logp, adv, ret, *cf)['ratio']
        for b in (1 - clip, 1 + clip):
            assert float((ratio - b).abs().min()) > 0.009
            for side in (ratio < b, ratio > b):
                near = side & ((ratio - b).abs() < 0.011)
                assert bool((near & (adv > 0)).any()) and bool((near & (adv < 0)).any()), (cset, b)
        assert bool((adv == 0).any())


def _coef_set_for(mut):
    # a coefficient set under which the mutation changes the result at all
    if mut in ('coefs_fixed_at_defaults', 'scale_fixed_at_1_over_M'):
        return 'B'
    return 'A'


@pytest.mark.parametrize('mut', sorted(R.MUTATIONS))
@pytest.mark.parametrize('D,M', [(160, 326), (138, 77)])
def test_checker_rejects_mutation(D, M, mut):
    stage = R.MUTATIONS[mut]
    res = _run(D, M, 'plain', _coef_set_for(mut), mut)
    print(D, M, mut, stage, round(res[stage], 1))
    assert res[stage] >= REJECT, (mut, stage, res)


@pytest.mark.parametrize('cset,mut', [('C', m) for m in R.ENTROPY_MUTATIONS] + [('B', 'entropy_total')])
def test_layer3_gradient_bound_rejects_entropy_mutations(cset, mut):
    """The case of the fused layer-3 gradient check (160, 512): an error in
    the entropy term overshoots the bound of dW3 or db3.  Under coefficient
    set C (ent_coef 1) all four do; under B (ent_coef 0.05) only the total
    entropy in place of the head's (20x / 98x).  The other three change 5 % of
    a gradient that is summed over 512 rows against a bound that sums the
    absolute per-row roundings, and reach (dW3 / db3) 0.6 / 1.2 (dropped),
    1.3 / 2.4 (sign) and 0.6 / 0.4 (last head missing): at ent_coef 0.05 only
    the per-row check of the same kernel body sees them (40x to 110x)."""
    res = _run(160, 512, 'plain', cset, mut)
    print(cset, mut, round(res['dw3'], 1), round(res['db3'], 1))
    assert max(res['dw3'], res['db3']) >= REJECT, (mut, res)


# --- the parameter gradients (policy_rows_ref.check_grads) ------------------

GRAD_SHAPES = [(160, 326), (138, 77), (160, 8192)]  # the last: ppo._split_k makes two chunks


@functools.lru_cache(maxsize=None)
def _grad_case(D, M):
    """(x with the ones column, the emulation's stored tensors, the chunk count)."""
    from masurvival.ppo import _split_k
    P, x, batch, cf = _case(D, M, 'plain', 'A')
    x1 = torch.cat([x.float(), torch.ones((M, 1))], 1)
    return x1, R.emulate(P, x, batch, cf), _split_k(M)


@functools.lru_cache(maxsize=None)
def _grads(D, M, mode, mut=None):
    x1, out, _ = _grad_case(D, M)
    return R.emulate_grads(x1, out, mode, mut, torch.Generator().manual_seed(M))


def test_split_k_chunks_of_the_gradient_shapes():
    assert [_grad_case(D, M)[2] for D, M in GRAD_SHAPES] == [1, 1, 2]


@pytest.mark.parametrize('D,M', GRAD_SHAPES)
def test_gradient_emulation_passes_the_checker(D, M):
    x1, out, chunks = _grad_case(D, M)
    fp32 = R.check_grads(x1, out, _grads(D, M, 'fp32'), gemm=(), chunks=chunks)
    gemm = R.check_grads(x1, out, _grads(D, M, 'gemm'), gemm=(1, 2, 3), chunks=chunks)
    print(D, M, 'fp32', {k: round(v, 3) for k, v in fp32.items()})
    print(D, M, 'gemm', {k: round(v, 3) for k, v in gemm.items()})
    for k in R.GRADS:
        assert fp32[k] <= 1.0, (k, fp32)
        assert gemm[k] <= 1.0, (k, gemm)
    # the layers mixed as FusedPolicy.grads mixes them: layer 1 a GEMM, 2 and 3 fp32 sums
    mixed = dict(_grads(D, M, 'fp32'), w1=_grads(D, M, 'gemm')['w1'], b1=_grads(D, M, 'gemm')['b1'])
    res = R.check_grads(x1, out, mixed, gemm=(1,), chunks=chunks)
    for k in R.GRADS:
        assert res[k] <= 1.0, (k, res)
    # without h2 and dz (the fused kernel stores neither) layer 3 is left out
    res = R.check_grads(x1, {k: out[k] for k in ('h1', 'da1', 'da2')}, mixed, gemm=(1,), chunks=chunks)
    assert sorted(k for k in res if k in R.GRADS) == ['b1', 'b2', 'w1', 'w2']


@pytest.mark.parametrize('mut', sorted(R.GRAD_MUTATIONS))
@pytest.mark.parametrize('mode', ['fp32', 'gemm'])
@pytest.mark.parametrize('D,M', [(160, 326), (138, 77)])
def test_gradient_checker_rejects_mutation(D, M, mode, mut):
    x1, out, chunks = _grad_case(D, M)
    res = R.check_grads(x1, out, _grads(D, M, mode, mut), gemm=(1, 2, 3) if mode == 'gemm' else (), chunks=chunks)
    print(D, M, mode, mut, {k: round(res[k], 2) for k in R.GRADS})
    for k in R.GRAD_MUTATIONS[mut]:
        assert res[k] > 1.0, (mut, k, res)


@pytest.mark.parametrize('D,M', GRAD_SHAPES)
def test_gemm_layer1_gradient_exceeds_the_fp32_bound(D, M):
    """dW1 through the bf16-output GEMM, declared an fp32 sum: rejected.  The
    rounding of the chunk products to bf16 is many times the fp32 bound (the
    figure printed; 65x / 20x / 11x on random operands at M = 512 / 8192 /
    16384), which is why check_grads carries BF16_HALF_ULP sum |S_c| for it."""
    x1, out, chunks = _grad_case(D, M)
    g = _grads(D, M, 'gemm')
    res = R.check_grads(x1, out, g, gemm=(), chunks=chunks)
    ok = R.check_grads(x1, out, g, gemm=(1, 2, 3), chunks=chunks)
    print(D, M, 'w1 over the fp32-only bound', round(res['w1'], 1), 'over the GEMM bound', round(ok['w1'], 3))
    assert res['w1'] > 1.0, res
    assert ok['w1_x_fp32'] == res['w1'] and ok['w1'] <= 1.0


def test_layer3_gradient_check_forced_on_the_stored_h2():
    """check_dw3 teacher-forced on the emulation's stored h2 (h2k): the clean
    sums pass, no row is granted a clip flip (make_batch keeps the ratios 0.01
    from the boundaries), the bound is the tighter one, and an entropy error
    is still rejected."""
    P, x, batch, cf = _case(160, 512, 'plain', 'C')
    out = R.emulate(P, x, batch, cf)
    un = R.check_dw3(P, x, batch, cf, out['dw3'], out['db3'])
    fo = R.check_dw3(P, x, batch, cf, out['dw3'], out['db3'], h2k=out['h2'])
    print('unforced', un, 'forced', fo)
    assert fo['flip_rows'] == 0 and fo['dw3'] <= 1.0 and fo['db3'] <= 1.0
    bad = R.emulate(P, x, batch, cf, 'entropy_sign')
    res = R.check_dw3(P, x, batch, cf, bad['dw3'], bad['db3'], h2k=bad['h2'])
    assert max(res['dw3'], res['db3']) >= REJECT, res
    # a row moved onto its clip boundary is granted its surrogate term, and only then
    acts, old_logp, adv, ret = batch
    z = out['h2'].double() @ P['W3'].T + P['b3']
    i = int(torch.nonzero(adv > 0)[0])
    lp2 = old_logp.clone()
    lp2[i] = float(R.log_prob(z, acts)[i] - torch.log(torch.tensor(1.0 + cf[0], dtype=torch.float64)))
    b2 = (acts, lp2, adv, ret)
    o2 = R.emulate(P, x, b2, cf)
    r2 = R.check_dw3(P, x, b2, cf, o2['dw3'], o2['db3'], h2k=o2['h2'])
    print('one row on the boundary', r2)
    assert r2['flip_rows'] == 1 and r2['dw3'] <= 1.0 and r2['db3'] <= 1.0
