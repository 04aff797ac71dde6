"""The argument checks of mas_obs_stats, mas_obs_norm_merge and
mas_policy_pack_norm come before any HIP call: they run here without a GPU, on
null or never-dereferenced device pointers."""
import ctypes

import pytest

from masurvival import abi

P, Q, R, S = 4096, 8192, 12288, 16384  # distinct, 16-B aligned, never dereferenced addresses
NAMES = ('mas_obs_stats_scratch_doubles', 'mas_obs_stats', 'mas_obs_norm_merge', 'mas_policy_pack_norm')


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _v(p):
    return ctypes.c_void_p(p)


def _stats(lib, n_rows=64, n_cols=138, x=P, x_stride=144, sums=Q, scratch=R):
    return lib.mas_obs_stats(n_rows, n_cols, _v(x), x_stride, _v(sums), _v(scratch), None)


def _merge(lib, n_cols=138, state=P, batch=Q, eps=1e-2, mean_out=R, inv_std_out=S):
    return lib.mas_obs_norm_merge(n_cols, _v(state), _v(batch), eps, _v(mean_out), _v(inv_std_out), None)


def _pack(lib, obs_dim=138, w1=P, b1=P, w2=P, b2=P, w3=P, b3=P, mean=Q, inv_std=R, packed=S):
    return lib.mas_policy_pack_norm(obs_dim, _v(w1), _v(b1), _v(w2), _v(b2), _v(w3), _v(b3), _v(mean), _v(inv_std),
                                    _v(packed), None)


def _invalid(lib, fn, name, word=None, **kw):
    assert fn(lib, **kw) == -1, kw
    msg = lib.mas_last_error().decode()
    assert msg.startswith(name + ':'), msg
    if word is not None:
        assert word in msg, msg


def test_symbols_are_declared_optional_and_present(lib):
    for name in NAMES:
        assert name in abi.SIGNATURES and name in abi.OPTIONAL, name
        assert hasattr(lib, name), name
    assert lib.mas_abi_version() == 3


@pytest.mark.parametrize('kw,word', [
    (dict(n_rows=-1), 'n_rows'),
    (dict(n_cols=0), 'n_cols'),
    (dict(n_cols=-3), 'n_cols'),
    (dict(n_cols=145), 'n_cols'),             # past x_stride
    (dict(x_stride=140), 'x_stride'),         # no multiple of 8
    (dict(x_stride=0), 'x_stride'),
    (dict(x=P + 8), 'x_bf16'),                # not 16-B aligned
    (dict(x=None), 'x_bf16'),                 # rows to read and nothing to read them from
    (dict(sums=None), 'null'),
    (dict(scratch=None), 'null'),
    (dict(sums=Q + 4), 'aligned'),
    (dict(scratch=R + 4), 'aligned'),
    (dict(n_rows=0, sums=None), 'null'),      # refused before the empty case returns
    (dict(n_rows=0, scratch=None), 'null'),
])
def test_obs_stats_refusals(lib, kw, word):
    _invalid(lib, _stats, 'mas_obs_stats', word, **kw)


def test_scratch_doubles(lib):
    f = lib.mas_obs_stats_scratch_doubles
    assert f(-1, 138) == -1 and f(64, 0) == -1 and f(64, -1) == -1
    assert f(0, 138) == 0
    one = f(1, 138)
    assert one >= 2 * 138          # one record holds both kinds of every column
    assert f(1, 8) == 16
    # the grid is capped: a million times the rows, a bounded scratch
    assert 0 < f(1 << 22, 138) < (1 << 20) and 0 < f(1 << 32, 138) < (1 << 20)
    # a function of (n_rows, n_cols) alone
    assert f(4099, 160) == f(4099, 160)


@pytest.mark.parametrize('kw,word', [
    (dict(n_cols=0), 'n_cols'),
    (dict(n_cols=-1), 'n_cols'),
    (dict(state=None), 'null'),
    (dict(batch=None), 'null'),
    (dict(mean_out=None), 'null'),
    (dict(inv_std_out=None), 'null'),
    (dict(state=P + 4), 'misaligned'),
    (dict(batch=Q + 4), 'misaligned'),
    (dict(mean_out=R + 2), 'misaligned'),
    (dict(inv_std_out=S + 1), 'misaligned'),
    (dict(eps=-1e-3), 'eps'),
    (dict(eps=float('nan')), 'eps'),
    (dict(eps=float('inf')), 'eps'),
])
def test_obs_norm_merge_refusals(lib, kw, word):
    _invalid(lib, _merge, 'mas_obs_norm_merge', word, **kw)


@pytest.mark.parametrize('kw,word', [
    (dict(obs_dim=0), None),
    (dict(w1=None), None), (dict(b1=None), None), (dict(w2=None), None), (dict(b2=None), None),
    (dict(w3=None), None), (dict(b3=None), None), (dict(packed=None), None),
    (dict(mean=None), 'both'),                # one of the two statistics missing
    (dict(inv_std=None), 'both'),
])
def test_policy_pack_norm_refusals(lib, kw, word):
    _invalid(lib, _pack, 'mas_policy_pack_norm', word, **kw)
