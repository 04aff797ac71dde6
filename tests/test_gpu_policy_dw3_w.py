"""mas_policy_train_dw3_w (the layer-3 weight gradient accumulated inside the
weighted train kernel, k_policy_train_db<.., DW3, RW>) against the weighted
unfused path (MAS_POL_DW3=0: mas_policy_train_w stores h2 and dz,
mas_policy_dw(16, 256) sums them), on the cases and with the criteria of
test_gpu_policy_dw3.py and {0, 1} row weights, about a third zeros: layers 1
and 2 bit-identical, layer 3 within 1e-5 (|dz| |h2|^T) + 1e-6 (weight) and
1e-5 sum |dz| + 1e-6 (bias) of the unfused sums and of a torch fp32 product of
the stored dz and h2, bit-identical where the fused kernel splits the rows as
mas_policy_dw does; h2 and dz neither read nor written; a partial block
refused with nothing written."""
import ctypes
import functools
import os

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import test_gpu_policy_dw3 as T3  # noqa: E402
from masurvival import ppo as ppo_mod  # noqa: E402
from masurvival.abi import MAS_ERR_UNSUPPORTED  # noqa: E402
from masurvival.ppo import PPOConfig  # noqa: E402


def _weights(M):
    g = torch.Generator(device='cuda').manual_seed(11)
    return (torch.rand(M, device='cuda', generator=g) >= 1.0 / 3.0).float()


def _grads(p, fp, batch, w, fused, poison=False):
    """test_gpu_policy_dw3._grads with row weights."""
    assert ppo_mod._POL_LAYOUT == 'fm' and '3' in ppo_mod._DW_LAYERS
    M = batch[0].shape[0]
    if poison:
        B = fp._buffers_l3(M)
        B['h2'].fill_(float('nan'))
        B['dz'].fill_(float('nan'))
    old = os.environ.get('MAS_POL_DW3')
    os.environ['MAS_POL_DW3'] = '1' if fused else '0'
    try:
        for q in p.parameters():
            q.grad = None
        terms = [float(t) for t in fp.grads(*batch, PPOConfig(), row_w=w)]
    finally:
        if old is None:
            del os.environ['MAS_POL_DW3']
        else:
            os.environ['MAS_POL_DW3'] = old
    torch.cuda.synchronize()
    grads = {n: q.grad.detach().clone() for n, q in p.named_parameters()}
    B = fp._bufs
    return terms, grads, ((B['h2'], B['dz']) if 'h2' in B else None)


@functools.lru_cache(maxsize=None)
def _both(case):
    D, M = T3._rows(case)
    w = _weights(M)
    p, fp, batch = T3._inputs(D, M)
    t0, g0, l3 = _grads(p, fp, batch, w, fused=False)
    h2, dz = l3
    dzf, h2f = dz[:, :M].float(), h2[:256, :M].float()
    p1, fp1, batch1 = T3._inputs(D, M)
    t1, g1, l3_1 = _grads(p1, fp1, batch1, w, fused=True)
    # the weights reached the kernel: the rows with w = 0 have no logit gradient
    assert bool((dzf[:15][:, w == 0] == 0).all()) and bool((dzf[:15][:, w != 0] != 0).any())
    return dict(M=M, t0=t0, g0=g0, t1=t1, g1=g1, dzf=dzf, h2f=h2f, stored1=l3_1 is not None)


@pytest.mark.parametrize('case', T3.FUSED_CASES)
def test_dw3_w_fused_matches_unfused(case):
    r = _both(case)
    assert not r['stored1'], 'the fused call allocated h2 / dz: it took the unfused path'
    for a, b in zip(r['t1'], r['t0']):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (r['t1'], r['t0'])
    for n in ('body.0.weight', 'body.0.bias', 'body.2.weight', 'body.2.bias'):
        assert torch.equal(r['g1'][n], r['g0'][n]), n
    dzf, h2f = r['dzf'], r['h2f']
    bound_w = 1e-5 * (dzf.abs() @ h2f.abs().T) + 1e-6
    bound_b = 1e-5 * dzf.abs().sum(1) + 1e-6
    ref_w, ref_b = dzf @ h2f.T, dzf.sum(1)
    for name, w, b in (('unfused', r['g0']['head.weight'], r['g0']['head.bias']), ('torch fp32', ref_w, ref_b)):
        dw = (r['g1']['head.weight'] - w).abs()
        db = (r['g1']['head.bias'] - b).abs()
        print(f'{case} vs {name}: max |dW3| / bound {float((dw / bound_w).max()):.3g}, '
              f'max |db3| / bound {float((db / bound_b).max()):.3g}')
        assert bool((dw <= bound_w).all()), (case, name)
        assert bool((db <= bound_b).all()), (case, name)


@pytest.mark.parametrize('case', ['one_block', 'dw_split'])
def test_dw3_w_fused_is_bit_identical_on_the_unfused_split(case):
    r = _both(case)
    assert not r['stored1']
    for n in r['g0']:
        assert torch.equal(r['g1'][n], r['g0'][n]), n


def test_dw3_w_partial_last_block_takes_the_unfused_path():
    r = _both('partial_last_block')
    assert r['stored1'], 'a minibatch with a partial last block must store h2 / dz'
    for a, b in zip(r['t1'], r['t0']):
        assert a == b, (r['t1'], r['t0'])
    for n in r['g0']:
        assert torch.equal(r['g1'][n], r['g0'][n]), n


@pytest.mark.parametrize('case', ['one_block', 'grid_stride'])
def test_dw3_w_fused_neither_reads_nor_writes_h2_dz_and_is_deterministic(case):
    D, M = T3._rows(case)
    w = _weights(M)
    p, fp, batch = T3._inputs(D, M)
    _, g1, l3 = _grads(p, fp, batch, w, fused=True, poison=True)
    h2, dz = l3
    assert bool(torch.isnan(h2).all()) and bool(torch.isnan(dz).all())
    for n, g in g1.items():
        assert bool(torch.isfinite(g).all()), n
    _, g2, _ = _grads(p, fp, batch, w, fused=True)
    for n in ('head.weight', 'head.bias'):
        assert torch.equal(g1[n], g2[n]), n
    r = _both(case)
    for n in ('head.weight', 'head.bias'):
        assert torch.equal(g1[n], r['g1'][n]), n


def test_dw3_w_all_ones_equals_the_unweighted_fused_call():
    D, M = T3._rows('ks9_two_workgroups')
    p, fp, batch = T3._inputs(D, M)
    _, g0, _ = T3._grads(p, fp, batch, fused=True)
    _, g1, _ = _grads(p, fp, batch, torch.ones(M, device='cuda'), fused=True)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


def test_dw3_w_entry_point_refuses_a_partial_block():
    D, M = 160, 256 + 32
    p, fp, (xb, acts, old_lp, adv, ret) = T3._inputs(D, M)
    B = fp._buffers(M)
    scratch, _ = fp._dw_buffers(16, M)
    out = torch.full((16 * 256 + 16,), 12345.0, device='cuda')
    w = _weights(M)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = fp.lib.mas_policy_train_dw3_w(ptr(fp.packed), D, M, ptr(xb), fp.Dx, ptr(acts), ptr(old_lp), ptr(adv),
                                       ptr(ret), ptr(w), 0.2, 0.5, 0.01, 1.0 / M, ptr(B['h1']), ptr(B['da1']),
                                       ptr(B['da2']), B['ld'], ptr(B['part']), ptr(out), ptr(scratch), None)
    torch.cuda.synchronize()
    assert rc == MAS_ERR_UNSUPPORTED
    assert bool((out == 12345.0).all())
