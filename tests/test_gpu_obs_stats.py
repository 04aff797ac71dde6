"""mas_obs_stats and mas_obs_norm_merge on the GPU against numpy fp64.

Shapes: rows in {1, 7, 259, 4099} (one lane, less than a pass, several passes
with a remainder, more than one workgroup) x (n_cols, x_stride) in {(138, 144),
(160, 176), (468, 480), (8, 8)} (a chunk that straddles n_cols, chunks past
n_cols that are never read, 59 of 60 chunks, one chunk per row), and once a
slice that starts at a row offset inside a larger buffer.

The bound needs no measurement: the GPU sum and the reference are both fp64
sums of exactly representable terms (bf16 -> double and x * x are exact) in
some order, so each is within (n - 1) 2^-53 sum|term| (1 + o(1)) of the true
sum and they differ by at most n_rows 2^-52 sum|term|."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import abi  # noqa: E402

ROWS = [1, 7, 259, 4099]
COLS = [(138, 144), (160, 176), (468, 480), (8, 8)]


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(n_rows, n_cols, x_stride, seed):
    """randn * 3 + a per-column offset up to 100, rounded to bf16; one
    all-constant column, one 0/1 column with a single 1, NaN in every column
    at or past n_cols."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n_rows, x_stride), generator=g) * 3 + torch.linspace(-100.0, 100.0, x_stride)
    x[:, 1 % n_cols] = 100.0
    x[:, 3 % n_cols] = 0.0
    x[n_rows // 2, 3 % n_cols] = 1.0
    x[:, n_cols:] = float('nan')
    return x.to(torch.bfloat16).cuda()


def _stats(lib, x, n_cols, sums=None, scratch=None, fill=None):
    n_rows, x_stride = x.shape[0], x.stride(0)
    need = int(lib.mas_obs_stats_scratch_doubles(n_rows, n_cols))
    assert need >= 0
    if scratch is None:
        scratch = torch.empty((max(need, 1),), dtype=torch.float64, device='cuda')
    if fill is not None:
        scratch.fill_(fill)
    if sums is None:
        sums = torch.full((2, n_cols), float('nan'), dtype=torch.float64, device='cuda')
    abi.check(lib.mas_obs_stats(n_rows, n_cols, _ptr(x), x_stride, _ptr(sums), _ptr(scratch), _stream()))
    return sums


def _check_against_numpy(x, n_cols, sums):
    xd = x[:, :n_cols].float().double().cpu().numpy()
    got = sums.cpu().numpy()
    assert np.isfinite(got).all()
    n = xd.shape[0]
    for kind, term in enumerate((xd, xd * xd)):
        ref = term.sum(0)
        bound = n * 2.0 ** -52 * np.abs(term).sum(0)
        err = np.abs(got[kind] - ref)
        assert (err <= bound).all(), (kind, float((err - bound).max()))


@pytest.mark.parametrize('n_cols,x_stride', COLS)
@pytest.mark.parametrize('n_rows', ROWS)
def test_obs_stats_against_numpy_and_deterministic(lib, n_rows, n_cols, x_stride):
    x = _rows(n_rows, n_cols, x_stride, seed=n_rows + n_cols)
    a = _stats(lib, x, n_cols)
    _check_against_numpy(x, n_cols, a)
    # the constant column and the single 1 are exact whatever the order
    assert float(a[0, 1 % n_cols]) == 100.0 * n_rows and float(a[1, 1 % n_cols]) == 1e4 * n_rows
    if n_cols > 3:
        assert float(a[0, 3]) == 1.0 and float(a[1, 3]) == 1.0
    # the same bits whatever the scratch held
    b = _stats(lib, x, n_cols, fill=float('nan'))
    assert torch.equal(a, b)


def test_obs_stats_on_a_slice_at_a_row_offset(lib):
    n_cols, x_stride = 138, 144
    big = _rows(259 + 40, n_cols, x_stride, seed=5)
    x = big[33:33 + 259]
    assert x.data_ptr() % 16 == 0 and x.data_ptr() != big.data_ptr()
    a = _stats(lib, x, n_cols)
    _check_against_numpy(x, n_cols, a)
    assert torch.equal(a, _stats(lib, x.clone(), n_cols))  # the rows around the slice do not count


def test_obs_stats_zero_rows_zero_fills(lib):
    x = _rows(4, 138, 144, seed=1)
    sums = _stats(lib, x[:0], 138)
    assert torch.equal(sums, torch.zeros_like(sums))


def _merge_np(state, batch, eps):
    """numpy restatement of mas_obs_norm_merge (include/masurvival.h)."""
    D = (state.size - 1) // 2
    count, nb = state[0], batch[0]
    mean, m2 = state[1:1 + D].copy(), state[1 + D:].copy()
    n = count + nb
    if nb > 0:
        mean_b = batch[1:1 + D] / nb
        m2_b = np.maximum(batch[1 + D:] - nb * mean_b * mean_b, 0.0)
        d = mean_b - mean
        mean = mean + d * nb / n
        m2 = m2 + m2_b + d * d * count * nb / n
        state = np.concatenate([[n], mean, m2])
    if n > 0:
        return state, mean.astype(np.float32), (1.0 / np.sqrt(m2 / n + eps)).astype(np.float32)
    return state, np.zeros(D, np.float32), np.ones(D, np.float32)


def _ulps(a, b):
    """Distance in fp32 steps between two float32 arrays of one sign pattern."""
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_merge_three_batches_identity_and_empty_batch(lib):
    D, stride, eps = 138, 144, 1e-2
    state = torch.zeros((1 + 2 * D,), dtype=torch.float64, device='cuda')
    batch = torch.zeros_like(state)
    mean = torch.full((D,), 7.0, device='cuda')
    inv = torch.full((D,), 7.0, device='cuda')

    def merge():
        abi.check(lib.mas_obs_norm_merge(D, _ptr(state), _ptr(batch), eps, _ptr(mean), _ptr(inv), _stream()))

    # an empty state and an empty batch: the identity, the state untouched
    merge()
    assert torch.equal(state, torch.zeros_like(state))
    assert torch.equal(mean, torch.zeros_like(mean)) and torch.equal(inv, torch.ones_like(inv))
    ref = np.zeros(1 + 2 * D)
    for k, n_rows in enumerate((259, 7, 4099)):
        x = _rows(n_rows, D, stride, seed=40 + k)
        batch[0] = float(n_rows)
        _stats(lib, x, D, sums=batch[1:].view(2, D))  # mas_obs_stats writes at batch + 1
        merge()
        ref, rmean, rinv = _merge_np(ref, batch.cpu().numpy(), eps)
    got = state.cpu().numpy()
    assert got[0] == 259 + 7 + 4099
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    assert _ulps(mean.cpu().numpy(), rmean).max() <= 1
    assert _ulps(inv.cpu().numpy(), rinv).max() <= 1
    assert float(inv.max()) <= 10.0 and float(inv[1]) == 10.0  # the constant column sits at the variance floor
    # n_b = 0 leaves the state as it is and still writes the outputs
    before, m0, i0 = state.clone(), mean.clone(), inv.clone()
    batch.zero_()
    mean.fill_(7.0)
    inv.fill_(7.0)
    merge()
    assert torch.equal(state, before) and torch.equal(mean, m0) and torch.equal(inv, i0)


def test_obsnorm_update_is_the_two_calls(lib):
    from masurvival.ppo import ObsNorm, merge_reference, obs_moments_reference
    D, stride = 160, 176
    on = ObsNorm(D, torch.device('cuda'))
    ref = torch.zeros((1 + 2 * D,), dtype=torch.float64)
    for k, n_rows in enumerate((259, 4099)):
        x = _rows(n_rows, D, stride, seed=60 + k)
        on.update(x)
        b = torch.cat([torch.tensor([float(n_rows)], dtype=torch.float64),
                       obs_moments_reference(x.cpu(), D).reshape(-1)])
        rmean, rinv = merge_reference(ref, b, 1e-2)
    torch.testing.assert_close(on.state.cpu(), ref, rtol=1e-12, atol=0)
    torch.testing.assert_close(on.mean.cpu(), rmean, rtol=2e-7, atol=0)
    torch.testing.assert_close(on.inv_std.cpu(), rinv, rtol=2e-7, atol=0)
