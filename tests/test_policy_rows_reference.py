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
