"""The layer-3 weight gradient accumulated inside the PPO train kernel
(mas_policy_train_dw3, k_policy_train_db<.., DW3>) against the unfused path
(MAS_POL_DW3=0: mas_policy_train_ld stores h2 and dz, mas_policy_dw(16, 256)
sums them) on the same seeded minibatch.

The fused kernel leaves the data path alone, so the layer-1 and layer-2
gradients are bit-identical.  Layer 3 sums the same bf16-rounded dz and h2 in
fp32 in another order: the bound is test_policy_dw_matches_fp32's,
|d| <= 1e-5 (|dz| |h2|^T) + 1e-6 for the weight and 1e-5 sum |dz| + 1e-6 for
the bias, taken from the dz and h2 the unfused run stored.

Where the fused kernel splits the rows over its workgroups as mas_policy_dw
does (the trainer's minibatches; here one block, and 2048 rows for each of
256 workgroups, the smallest such minibatch that fills 256 CUs) it sums in
the unfused path's order and layer 3 is bit-identical too.

Shapes: one 256-row block on one workgroup; two workgroups with 9 layer-1
k-steps (D = 138); CUs + 3 blocks (a grid-stride loop with uneven blocks per
workgroup, the stage-buffer parity flipping per block); a partial last block
(the call must take the unfused path)."""
import ctypes
import functools
import os

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import ppo as ppo_mod  # noqa: E402
from masurvival.abi import MAS_ERR_UNSUPPORTED  # noqa: E402
from masurvival.ppo import FusedPolicy, PolicyMLP, PPOConfig  # noqa: E402


def _rows(case):
    if case == 'one_block':
        return 160, 256
    if case == 'ks9_two_workgroups':
        return 138, 512
    if case == 'grid_stride':
        return 160, 256 * (torch.cuda.get_device_properties(0).multi_processor_count + 3)
    if case == 'dw_split':
        return 160, 2048 * 256
    assert case == 'partial_last_block'
    return 160, 256 * 2 + 70


FUSED_CASES = ['one_block', 'ks9_two_workgroups', 'grid_stride', 'dw_split']


def _inputs(D, M):
    """A policy and one seeded minibatch, as test_policy_train_gradients_match_reference builds them."""
    torch.manual_seed(D + 1)
    p = PolicyMLP(D, 256).cuda()
    fp = FusedPolicy(p, D, torch.device('cuda'))
    fp.pack()
    g = torch.Generator(device='cuda').manual_seed(7)
    obs = torch.randn((M, D), device='cuda', generator=g) * 2.0
    xb = fp.x_buffer(M)
    acts = torch.empty((M, 6), dtype=torch.int8, device='cuda')
    lp = torch.empty((M,), device='cuda')
    v = torch.empty((M,), device='cuda')
    fp.act(obs, 1, 2, acts, lp, v, xb=xb)
    old_lp = lp + 0.3 * torch.randn((M,), device='cuda', generator=g)
    adv = torch.randn((M,), device='cuda', generator=g)
    ret = v + torch.randn((M,), device='cuda', generator=g)
    return p, fp, (xb, acts, old_lp, adv, ret)


def _grads(p, fp, batch, fused, poison=False):
    """One FusedPolicy.grads call with MAS_POL_DW3 set for it: (loss terms,
    gradients by parameter name, the h2 / dz buffers or None)."""
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
        terms = [float(t) for t in fp.grads(*batch, PPOConfig())]
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
    """The unfused and the fused run of a case, computed once for the tests that share them."""
    D, M = _rows(case)
    p, fp, batch = _inputs(D, M)
    t0, g0, l3 = _grads(p, fp, batch, fused=False)
    h2, dz = l3
    dzf, h2f = dz[:, :M].float(), h2[:256, :M].float()
    p1, fp1, batch1 = _inputs(D, M)
    t1, g1, l3_1 = _grads(p1, fp1, batch1, fused=True)
    return dict(M=M, t0=t0, g0=g0, t1=t1, g1=g1, dzf=dzf, h2f=h2f, stored1=l3_1 is not None)


@pytest.mark.parametrize('case', FUSED_CASES)
def test_dw3_fused_matches_unfused(case):
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
def test_dw3_fused_is_bit_identical_on_the_unfused_split(case):
    r = _both(case)
    assert not r['stored1']
    for n in r['g0']:
        assert torch.equal(r['g1'][n], r['g0'][n]), n


def test_dw3_partial_last_block_takes_the_unfused_path():
    r = _both('partial_last_block')
    assert r['stored1'], 'a minibatch with a partial last block must store h2 / dz'
    for a, b in zip(r['t1'], r['t0']):
        assert a == b, (r['t1'], r['t0'])
    for n in r['g0']:
        assert torch.equal(r['g1'][n], r['g0'][n]), n


@pytest.mark.parametrize('case', ['one_block', 'grid_stride'])
def test_dw3_fused_neither_reads_nor_writes_h2_dz_and_is_deterministic(case):
    D, M = _rows(case)
    p, fp, batch = _inputs(D, M)
    _, g1, l3 = _grads(p, fp, batch, fused=True, poison=True)
    h2, dz = l3
    assert bool(torch.isnan(h2).all()) and bool(torch.isnan(dz).all())
    for n, g in g1.items():
        assert bool(torch.isfinite(g).all()), n
    _, g2, _ = _grads(p, fp, batch, fused=True)
    for n in ('head.weight', 'head.bias'):
        assert torch.equal(g1[n], g2[n]), n
    # the same sums as the cached fused run of a fresh policy object
    r = _both(case)
    for n in ('head.weight', 'head.bias'):
        assert torch.equal(g1[n], r['g1'][n]), n


def test_dw3_entry_point_refuses_a_partial_block():
    D, M = 160, 256 + 32
    p, fp, (xb, acts, old_lp, adv, ret) = _inputs(D, M)
    B = fp._buffers(M)
    scratch, _ = fp._dw_buffers(16, M)
    out = torch.full((16 * 256 + 16,), 12345.0, device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = fp.lib.mas_policy_train_dw3(ptr(fp.packed), D, M, ptr(xb), fp.Dx, ptr(acts), ptr(old_lp), ptr(adv), ptr(ret),
                                     0.2, 0.5, 0.01, 1.0 / M, ptr(B['h1']), ptr(B['da1']), ptr(B['da2']), B['ld'],
                                     ptr(B['part']), ptr(out), ptr(scratch), None)
    torch.cuda.synchronize()
    assert rc == MAS_ERR_UNSUPPORTED
    assert bool((out == 12345.0).all())
