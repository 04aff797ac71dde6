"""The checker of the PPO optimizer step (tests/update_ref.py) on the CPU:
adam_ref is torch.optim.Adam + clip_grad_norm_ on fp64 tensors to 1e-12, the
fp32 emulation of the kernel passes the derived bound at every size class of
the kernel's launch (one element, a partial block, one element into a second
block, three elements into the grid-stride second pass, the D = 468 policy),
and every named error of the emulation is rejected at the D = 468 size."""
import functools

import numpy as np
import pytest
import torch

import update_ref as UR

LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-5
SIZES = [1, 255, 257, 131075, 189968]
# (step, max_norm, grad_scale): the clip active, no clip (max_norm <= 0), the clip inactive
REGIMES = [(1, 0.5, 1.0), (2, 0.0, 1.0), (1000, 1e9, 0.125), (2, 0.5, 0.125), (1000, 0.5, 1.0), (1, 1e9, 0.125)]


@functools.lru_cache(maxsize=None)
def _state(n, step, g_std=0.05, seed=3):
    """fp32 (p, g, m, v): every 7th gradient exactly 0; at step 1 both moments
    zero, else what earlier steps of such gradients leave (m ~ g, v ~ g^2)."""
    r = np.random.default_rng(seed + n)
    p = (0.1 * r.standard_normal(n)).astype(np.float32)
    g = (g_std * r.standard_normal(n)).astype(np.float32)
    g[::7] = 0.0
    if step == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    g1 = g_std * r.standard_normal(n)
    k = min(step - 1, 1000)
    m = ((1.0 - 0.9 ** k) * 0.3 * g1).astype(np.float32)
    v = ((1.0 - 0.999 ** k) * g1 * g1).astype(np.float32)
    return p, g, m, v


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('step,max_norm,grad_scale', REGIMES)
def test_emulation_passes_the_checker(n, step, max_norm, grad_scale):
    p, g, m, v = _state(n, step)
    assert bool((g[::7] == 0.0).all())
    args = (p, g, m, v, grad_scale, max_norm, LR, BETAS, EPS, step)
    res = UR.check_adam(*args, *UR.adam_emulate(*args))
    print(n, step, max_norm, grad_scale, {k: round(x, 3) for k, x in res.items()})
    for k in 'pmv':
        assert res[k] <= 1.0, (k, res)


def test_both_clip_regimes_are_reached():
    """The regimes above: max_norm 0.5 clips the n = 189968 gradient (its norm is
    about 20) and not the one-element one scaled by 0.125; 1e9 never clips."""
    t = UR._terms(*_state(189968, 2), 1.0, 0.5, LR, BETAS, EPS, 2)
    assert t['coef'] < 0.1
    assert UR._terms(*_state(189968, 2), 0.125, 1e9, LR, BETAS, EPS, 2)['coef'] == 1.0
    assert UR._terms(*_state(189968, 2), 1.0, 0.0, LR, BETAS, EPS, 2)['coef'] == 1.0


# The mutations at n = 189968, step 2.  Those of the clip coefficient need the
# clip active and a small norm (1e-6 against the norm is what the missing
# constant changes: at norm 0.02 it is 5e-5, ten times the fp32 norm error the
# bound grants); the others run without the clip, so that EC does not hide them.
def _mutation_case(mut):
    if mut in ('coef_without_1e-6', 'norm_of_unscaled_grad'):
        return _state(189968, 2, g_std=4e-4), 0.125, 0.01
    return _state(189968, 2), 1.0, 1e9


@pytest.mark.parametrize('mut', UR.MUTATIONS)
def test_checker_rejects_mutation(mut):
    (p, g, m, v), grad_scale, max_norm = _mutation_case(mut)
    args = (p, g, m, v, grad_scale, max_norm, LR, BETAS, EPS, 2)
    clean = UR.check_adam(*args, *UR.adam_emulate(*args))
    res = UR.check_adam(*args, *UR.adam_emulate(*args, mut=mut))
    print(mut, {k: round(x, 2) for k, x in res.items()}, 'clean', {k: round(x, 3) for k, x in clean.items()})
    assert max(clean.values()) <= 1.0, clean
    assert max(res.values()) > 1.0, (mut, res)
    if mut in ('coef_without_1e-6', 'norm_of_unscaled_grad'):
        assert UR._terms(*args)['coef'] < 1.0


@pytest.mark.parametrize('n', [1, 257, 4099])
@pytest.mark.parametrize('step,max_norm,grad_scale', REGIMES)
def test_adam_ref_is_torch_adam_in_fp64(n, step, max_norm, grad_scale):
    p, g, m, v = (torch.from_numpy(a).double() for a in _state(n, step))
    prm = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([prm], lr=LR, betas=BETAS, eps=EPS)
    opt.state[prm] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
    prm.grad = g * grad_scale
    if max_norm > 0.0:
        torch.nn.utils.clip_grad_norm_([prm], max_norm)
    opt.step()
    st = opt.state[prm]
    assert float(st['step']) == step
    ref = UR.adam_ref(p.numpy(), g.numpy(), m.numpy(), v.numpy(), grad_scale, max_norm, LR, BETAS, EPS, step)
    for name, a, b in zip('pmv', ref, (prm.detach(), st['exp_avg'], st['exp_avg_sq'])):
        b = b.numpy()
        assert bool((np.abs(a - b) <= 1e-12 * np.abs(b)).all()), (name, float(np.abs(a - b).max()))
