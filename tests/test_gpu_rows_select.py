"""mas_rows_select (masurvival.ppo.rows_select): the dense gather of the
bit-selected agents' rows, against torch indexing of the same inputs.

A copy, not arithmetic: the inputs are random bit patterns (NaN patterns
included) and every comparison is torch.equal on integer views.  Outputs are
pre-filled with canaries: the columns of x_out past x_cols, a guard region
past the last output row, and the outputs of pairs a call leaves out must
keep them."""
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import rows_select  # noqa: E402

DEV = 'cuda'
GUARD = 3            # rows past the last output row
X_CANARY = 0x5A5A    # int16 view of the bf16 outputs
A_CANARY = -7
F_CANARY = 0x7FC0BEEF  # a quiet NaN with a payload

CASES = [(4, 0b0011), (4, 0b1010), (4, 0b1111), (2, 0b10), (1, 0b1), (8, 0b10010110), (32, 0x80000001)]


def _agents(mask):
    return [a for a in range(32) if (mask >> a) & 1]


def _index(n_envs, A, mask):
    """Input row of every output row, in (env, ascending agent) order."""
    ag = torch.tensor(_agents(mask), dtype=torch.long)
    return (torch.arange(n_envs).unsqueeze(1) * A + ag.unsqueeze(0)).reshape(-1).to(DEV)


def _inputs(rows, stride, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-32768, 32768, (rows, stride), dtype=torch.int16, generator=g)
    x[0, :4] = torch.tensor([0x7FC1, 0x7F81, -1, -128], dtype=torch.int16)  # quiet / signalling NaN, -NaN, ...
    a = torch.randint(-128, 128, (rows, 6), dtype=torch.int8, generator=g)
    f = [torch.randint(-2 ** 31, 2 ** 31, (rows,), dtype=torch.int32, generator=g) for _ in range(4)]
    return x.to(DEV).view(torch.bfloat16), a.to(DEV), [t.to(DEV).view(torch.float32) for t in f]


def _outputs(n_out, out_stride):
    x = torch.full((n_out + GUARD, out_stride), X_CANARY, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    a = torch.full((n_out + GUARD, 6), A_CANARY, dtype=torch.int8, device=DEV)
    f = [torch.full((n_out + GUARD,), F_CANARY, dtype=torch.int32, device=DEV).view(torch.float32) for _ in range(4)]
    return x, a, f


def _i16(t):
    return t.view(torch.int16)


def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('stride', [144, 176, 480])
@pytest.mark.parametrize('n_envs', [1, 37, 1000])
@pytest.mark.parametrize('A,mask', CASES)
def test_gather_equals_torch_indexing(A, mask, n_envs, stride):
    m = len(_agents(mask))
    rows, n_out = n_envs * A, n_envs * m
    x, a, f = _inputs(rows, stride, seed=stride + n_envs + A)
    x0, a0, f0 = x.clone(), a.clone(), [t.clone() for t in f]
    # x_cols below the input stride at 480 (the input's last columns are not copied), the whole row otherwise
    x_cols = stride - 16 if stride == 480 else stride
    xo, ao, fo = _outputs(n_out, stride + 8)
    rows_select(A, mask, x=x, x_out=xo[:n_out], x_cols=x_cols, actions=a, actions_out=ao[:n_out],
                f32=[(t, o[:n_out]) for t, o in zip(f, fo)])
    torch.cuda.synchronize()
    idx = _index(n_envs, A, mask)
    assert torch.equal(_i16(xo)[:n_out, :x_cols], _i16(x)[idx][:, :x_cols])
    assert bool((_i16(xo)[:n_out, x_cols:] == X_CANARY).all())
    assert bool((_i16(xo)[n_out:] == X_CANARY).all())
    assert torch.equal(ao[:n_out], a[idx]) and bool((ao[n_out:] == A_CANARY).all())
    for t, o in zip(f, fo):
        assert torch.equal(_i32(o)[:n_out], _i32(t)[idx]) and bool((_i32(o)[n_out:] == F_CANARY).all())
    # the inputs are not written
    assert torch.equal(_i16(x), _i16(x0)) and torch.equal(a, a0)
    assert all(torch.equal(_i32(t), _i32(t0)) for t, t0 in zip(f, f0))


@pytest.mark.parametrize('given', ['x', 'actions', 'f32_one', 'f32_three'])
def test_pairs_left_out_stay_untouched(given):
    A, mask, n_envs, stride = 4, 0b0110, 37, 176
    n_out = n_envs * 2
    x, a, f = _inputs(n_envs * A, stride, seed=5)
    xo, ao, fo = _outputs(n_out, stride)
    idx = _index(n_envs, A, mask)
    kw = {'x': dict(x=x, x_out=xo[:n_out]), 'actions': dict(actions=a, actions_out=ao[:n_out]),
          'f32_one': dict(f32=[(f[1], fo[1][:n_out])]),
          'f32_three': dict(f32=[(f[k], fo[k][:n_out]) for k in (0, 2, 3)])}[given]
    rows_select(A, mask, **kw)
    torch.cuda.synchronize()
    if given == 'x':
        assert torch.equal(_i16(xo)[:n_out], _i16(x)[idx])
    else:
        assert bool((_i16(xo) == X_CANARY).all())
    if given == 'actions':
        assert torch.equal(ao[:n_out], a[idx])
    else:
        assert bool((ao == A_CANARY).all())
    written = {'f32_one': (1,), 'f32_three': (0, 2, 3)}.get(given, ())
    for k in range(4):
        if k in written:
            assert torch.equal(_i32(fo[k])[:n_out], _i32(f[k])[idx]) and bool((_i32(fo[k])[n_out:] == F_CANARY).all())
        else:
            assert bool((_i32(fo[k]) == F_CANARY).all())


@pytest.mark.parametrize('A,mask,n_envs', [(4, 0b0011, 37), (8, 0b10010110, 1000), (32, 0x80000001, 37), (2, 0b10, 1)])
def test_complementary_masks_reassemble_the_input(A, mask, n_envs):
    stride = 176
    other = ((1 << A) - 1) ^ mask
    rows = n_envs * A
    x, a, f = _inputs(rows, stride, seed=A + n_envs)
    bx = torch.zeros_like(x)
    ba = torch.zeros_like(a)
    bf = torch.zeros_like(f[0])
    for msk in (mask, other):
        n_out = n_envs * len(_agents(msk))
        xo, ao, fo = _outputs(n_out, stride)
        rows_select(A, msk, x=x, x_out=xo[:n_out], actions=a, actions_out=ao[:n_out], f32=[(f[0], fo[0][:n_out])])
        idx = _index(n_envs, A, msk)
        _i16(bx)[idx] = _i16(xo)[:n_out]
        ba[idx] = ao[:n_out]
        _i32(bf)[idx] = _i32(fo[0])[:n_out]
    assert torch.equal(_i16(bx), _i16(x)) and torch.equal(ba, a) and torch.equal(_i32(bf), _i32(f[0]))


def test_offsets_past_2_to_the_31_elements():
    """Row offsets of the input pass 2^31 elements (4.3 GB of bf16): 64-bit
    offsets throughout.  Generated on the device; agent 1 of 2 selected."""
    A, stride, n_envs = 2, 480, 2_240_000  # rows * stride = 2.15e9 > 2^31
    rows = n_envs * A
    assert rows * stride > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(-32768, 32768, (rows, stride), dtype=torch.int16, device=DEV, generator=g).view(torch.bfloat16)
    xo = torch.full((n_envs + GUARD, stride), X_CANARY, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    rows_select(A, 0b10, x=x, x_out=xo[:n_envs])
    torch.cuda.synchronize()
    assert torch.equal(_i16(xo)[:n_envs], _i16(x).view(n_envs, A, stride)[:, 1])
    assert bool((_i16(xo)[n_envs:] == X_CANARY).all())


@pytest.mark.parametrize('bad', ['host_x', 'host_out', 'x_dtype', 'actions_dtype', 'f32_dtype', 'rows', 'out_rows',
                                 'strided_actions', 'mask_zero', 'mask_high', 'self'])
def test_wrapper_refuses_wrong_tensors_before_the_device(bad):
    A, mask, n_envs, stride = 4, 0b0011, 8, 176
    n_out = n_envs * 2
    x, a, f = _inputs(n_envs * A, stride, seed=9)
    xo, ao, fo = _outputs(n_out, stride)
    kw = dict(x=x, x_out=xo[:n_out], actions=a, actions_out=ao[:n_out], f32=[(f[0], fo[0][:n_out])])
    if bad == 'host_x':
        kw['x'] = x.cpu()
    elif bad == 'host_out':
        kw['f32'] = [(f[0], fo[0][:n_out].cpu())]
    elif bad == 'x_dtype':
        kw['x'] = x.view(torch.float16)
    elif bad == 'actions_dtype':
        kw['actions'] = a.view(torch.uint8)
    elif bad == 'f32_dtype':
        kw['f32'] = [(f[0].double(), fo[0][:n_out])]
    elif bad == 'rows':
        kw['x'] = x[:-1]  # not whole envs
        kw['actions'], kw['f32'] = a[:-1], [(f[0][:-1], fo[0][:n_out])]
    elif bad == 'out_rows':
        kw['actions_out'] = ao[:n_out + 1]
    elif bad == 'strided_actions':
        kw['actions'] = torch.zeros((n_envs * A, 12), dtype=torch.int8, device=DEV)[:, ::2]
    elif bad == 'mask_zero':
        mask = 0
    elif bad == 'mask_high':
        mask = 0b10000
    elif bad == 'self':
        kw['f32'] = [(f[0], f[0])]
    with pytest.raises(ValueError, match='rows_select'):
        rows_select(A, mask, **kw)
    torch.cuda.synchronize()
    assert bool((_i16(xo) == X_CANARY).all()) and bool((ao == A_CANARY).all())
    assert bool((_i32(fo[0]) == F_CANARY).all())
