"""The six .grad tensors a FusedPolicy.grads call ends with, element by element
against the fp64 sums over the rows of what the call's own train kernel stored
(tests/policy_rows_ref.py check_grads; layer 3 of the fused kernel, which
stores neither h2 nor dz, against the unforced chain: check_dw3), on every
assembly path of grads():

  fused      mas_policy_train_dw3 writes dW3; mas_policy_dw layer 2; _splitk_nn layer 1
  unfused    MAS_POL_DW3=0: mas_policy_train_ld, mas_policy_dw for layers 2 and 3
  refused    the fused entry point answers MAS_ERR_UNSUPPORTED (a partial last
             block, or a layer-1 depth it has no instantiation for) and the call
             falls through to the unfused one; M % 32 != 0: _splitk_nt
  rm         MAS_POL_LAYOUT=rm: _grads_rm, three _splitk_tn GEMMs un-permuted
  weighted   row_w, fused and unfused

Each feature-major case runs twice, with .grad unset (scratch outputs, copies)
and under a FusedAdam (the kernels write into its flat gradient buffer): both
pass the checker and are bit-identical, tensor by tensor and as the whole flat
buffer.  The bounds are policy_rows_ref's: the fp32 one for mas_policy_dw and
the in-kernel dW3, plus the bf16 rounding of the chunk products for the torch
GEMMs (layer 1 always).  The figures measured on the MI355X are in
profiles/update_check.txt."""
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import policy_rows_ref as R  # noqa: E402
import test_gpu_policy_dw3_w as TW  # noqa: E402
import test_gpu_policy_rows as TR  # noqa: E402
from masurvival import ppo as ppo_mod  # noqa: E402
from masurvival.ppo import FusedAdam, PPOConfig  # noqa: E402

NAMES = {'w1': 'body.0.weight', 'b1': 'body.0.bias', 'w2': 'body.2.weight', 'b2': 'body.2.bias',
         'w3': 'head.weight', 'b3': 'head.bias'}

# case -> (path, D, M (0: the grid-stride size), layers summed by a torch GEMM, row weights)
CASES = {
    # one block, two blocks (9 layer-1 k-steps), 32 blocks and two layer-1 chunks, uneven blocks per workgroup
    'fused-160-256': ('fused', 160, 256, (1,), False),
    'fused-138-512': ('fused', 138, 512, (1,), False),
    'fused-160-8192': ('fused', 160, 8192, (1,), False),
    'fused-160-grid_stride': ('fused', 160, 0, (1,), False),
    # k_dw_lds on one split block; two split blocks, the second uneven; k_dw_nt (544 = 32 * 17)
    'unfused-160-512': ('unfused', 160, 512, (1,), False),
    'unfused-160-4160': ('unfused', 160, 4160, (1,), False),
    'unfused-160-544': ('unfused', 160, 544, (1,), False),
    # a partial last block: refused; with mas_policy_dw (576 = 64 * 9) and with the GEMMs (M % 32 = 6, odd M)
    'refused-160-576': ('refused', 160, 576, (1,), False),
    'refused-160-582': ('refused', 160, 582, (1, 2, 3), False),
    'refused-160-326': ('refused', 160, 326, (1, 2, 3), False),
    'refused-138-77': ('refused', 138, 77, (1, 2, 3), False),
    # the generic layer-1 k-loop (no fused instantiation: refused)
    'refused-468-130': ('refused', 468, 130, (1, 2, 3), False),
    'refused-468-512': ('refused', 468, 512, (1,), False),
    'rm-160-326': ('rm', 160, 326, (1, 2, 3), False),
    'rm-138-77': ('rm', 138, 77, (1, 2, 3), False),
    'fused_w-160-512': ('fused', 160, 512, (1,), True),
    'unfused_w-160-512': ('unfused', 160, 512, (1,), True),
}
FM_CASES = [c for c, v in CASES.items() if v[0] != 'rm']


def _setenv(monkeypatch, path):
    for k in ('MAS_POL_DB', 'MAS_POL_CW', 'MAS_POL_FORCE_OFF64', 'MAS_POL_DW3'):
        monkeypatch.delenv(k, raising=False)
    if path == 'unfused':
        monkeypatch.setenv('MAS_POL_DW3', '0')
    assert ppo_mod._DW_LAYERS == '23'


def _stored(fp, M):
    """What the last grads call stored, [M, F] fp32 in natural feature order."""
    B = fp._bufs
    assert B['M'] == M
    if fp.layout == 'rm':
        q = fp._rm_q  # feature -> stored column
        out = {k: B[k][:M, :256].index_select(1, q) for k in ('h1', 'h2', 'da1', 'da2')}
        out['dz'] = B['dz'][:M]
    else:
        out = {k: B[k][:256, :M].T for k in ('h1', 'h2', 'da1', 'da2') if k in B}
        if 'dz' in B:
            out['dz'] = B['dz'][:, :M].T
    return {k: v.float() for k, v in out.items()}


def _run(case, monkeypatch, span, stats=True):
    """One FusedPolicy.grads call of `case` (span: under a FusedAdam, so that
    .grad are views of its flat buffer) and its check.  Returns (ratios, the
    six gradients as clones, the flat gradient buffer or None, grads' result)."""
    path, D, M, gemm, weighted = CASES[case]
    M = M or TR._grid_stride_rows()
    _setenv(monkeypatch, path)
    p, fp = TR._policy(D, 'plain', path == 'rm', monkeypatch)
    fa = None
    if span:
        opt = torch.optim.Adam(p.parameters(), lr=3e-4, eps=1e-5)
        fa = FusedAdam(p.parameters(), opt, fp.lib, torch.device('cuda'))
        fp.pack()
        assert fp._grad_span(p.head.weight, p.head.bias) is not None
    else:
        assert all(q.grad is None for q in p.parameters())
    P = R.params(p)
    xb, g = TR._rows(fp, D, M)
    x = xb[:, :D]
    cf = R.coef('A', M)
    cfg = PPOConfig()
    assert (cfg.clip, cfg.vf_coef, cfg.ent_coef) == cf[:3]
    w = TW._weights(M) if weighted else None
    stores_l3 = path != 'fused'
    h2 = None
    if stores_l3:
        # h2 does not depend on the batch: a first call on a null batch yields the kernel's own (make_batch)
        null = (torch.zeros((M, 6), dtype=torch.int8, device='cuda'),) + tuple(torch.zeros(M, device='cuda')
                                                                                for _ in range(3))
        fp.grads(xb, *null, cfg, row_w=w)
        h2 = _stored(fp, M)['h2']
        if not span:
            for q in p.parameters():
                q.grad = None
    batch = R.make_batch(P, x, cf, g, h2=h2)
    ret = fp.grads(xb, *batch, cfg, stats=stats, row_w=w)
    torch.cuda.synchronize()
    out = _stored(fp, M)
    assert ('h2' in out) == stores_l3, 'the call took the other train entry point'
    grads = {k: dict(p.named_parameters())[n].grad for k, n in NAMES.items()}
    for k, t in grads.items():
        assert bool(torch.isfinite(t).all()), k
    res = R.check_grads(xb[:, :D + 1], out, grads, gemm=gemm, chunks=ppo_mod._split_k(M))
    if not stores_l3:
        r3 = R.check_dw3(P, x, batch, cf, grads['w3'], grads['b3'], row_w=w)
        res['w3'], res['b3'] = r3['dw3'], r3['db3']
    if w is not None:  # the weights reached the kernel
        L = R.loss_rows(R.forward(P, x)[2], *batch, *cf, row_w=w)
        assert bool((L['dz'][w == 0][:, :15] == 0).all()) and bool((L['dz'][w != 0][:, :15] != 0).any())
        if 'dz' in out:
            assert bool((out['dz'][w == 0][:, :15] == 0).all())
    return res, {k: t.detach().clone() for k, t in grads.items()}, (fa.g.clone() if fa is not None else None), ret


def _report(case, span, res):
    M = CASES[case][2] or TR._grid_stride_rows()
    print(f'{case} M={M} {"span" if span else "copy"}: ' + ' '.join(f'{k} {res[k]:.3f}' for k in R.GRADS)
          + ' | over the fp32-only bound: ' + ' '.join(f'{k} {v:.1f}' for k, v in res.items() if k.endswith('_x_fp32')))


@pytest.mark.parametrize('case', FM_CASES)
def test_grads_match_fp64_sums_of_the_stored_rows(case, monkeypatch):
    r0, g0, _, st0 = _run(case, monkeypatch, span=False)
    _report(case, False, r0)
    r1, g1, flat, st1 = _run(case, monkeypatch, span=True)
    _report(case, True, r1)
    for k in R.GRADS:
        assert r0[k] <= 1.0, (k, r0)
        assert r1[k] <= 1.0, (k, r1)
    for k in R.GRADS:
        assert torch.equal(g0[k], g1[k]), k
    # the flat buffer is the six tensors in parameter order and nothing else: no in-place write reached a neighbour
    assert torch.equal(flat, torch.cat([g0[k].reshape(-1) for k in R.GRADS]))
    assert [float(a) for a in st0] == [float(a) for a in st1]


@pytest.mark.parametrize('case', [c for c, v in CASES.items() if v[0] == 'rm'])
def test_grads_row_major_match_fp64_sums_of_the_stored_rows(case, monkeypatch):
    res, _, _, _ = _run(case, monkeypatch, span=False)
    _report(case, False, res)
    for k in R.GRADS:
        assert res[k] <= 1.0, (k, res)


@pytest.mark.parametrize('case', ['fused-138-512', 'unfused-160-544'])
@pytest.mark.parametrize('span', [False, True])
def test_grads_without_stats_are_the_same_gradients(case, span, monkeypatch):
    _, g0, _, st0 = _run(case, monkeypatch, span=span)
    _, g1, _, st1 = _run(case, monkeypatch, span=span, stats=False)
    assert st1 is None and len(st0) == 5
    for k in R.GRADS:
        assert torch.equal(g0[k], g1[k]), k
