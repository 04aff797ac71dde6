"""The argument checks of mas_policy_train_w, mas_policy_train_dw3_w and
mas_alive come before any HIP call: they run here without a GPU, on null or
never-dereferenced device pointers."""
import ctypes

import pytest

from masurvival import abi

P = 4096  # a non-null, 16-B aligned "device pointer" that is never dereferenced


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _train_w(lib, packed=P, obs_dim=160, n_rows=512, x=P, x_stride=176, acts=P, old_logp=P, adv=P, ret=P, row_w=P,
             h1=P, h2=P, da1=P, da2=P, dz=P, ld=576, part=P):
    v = ctypes.c_void_p
    return lib.mas_policy_train_w(v(packed), obs_dim, n_rows, v(x), x_stride, v(acts), v(old_logp), v(adv), v(ret),
                                  v(row_w), 0.2, 0.5, 0.01, 1.0 / 512, v(h1), v(h2), v(da1), v(da2), v(dz), ld,
                                  v(part), None)


def _train_dw3_w(lib, packed=P, obs_dim=160, n_rows=512, x=P, x_stride=176, acts=P, old_logp=P, adv=P, ret=P,
                 row_w=P, h1=P, da1=P, da2=P, ld=576, part=P, out=P, scratch=P):
    v = ctypes.c_void_p
    return lib.mas_policy_train_dw3_w(v(packed), obs_dim, n_rows, v(x), x_stride, v(acts), v(old_logp), v(adv),
                                      v(ret), v(row_w), 0.2, 0.5, 0.01, 1.0 / 512, v(h1), v(da1), v(da2), ld,
                                      v(part), v(out), v(scratch), None)


def test_symbols_are_declared_optional_and_present(lib):
    for name in ('mas_policy_train_w', 'mas_policy_train_dw3_w', 'mas_alive'):
        assert name in abi.SIGNATURES and name in abi.OPTIONAL
        assert hasattr(lib, name)
    assert lib.mas_abi_version() == 3


@pytest.mark.parametrize('call,name', [(_train_w, 'mas_policy_train_w'), (_train_dw3_w, 'mas_policy_train_dw3_w')])
def test_null_or_misaligned_row_w_is_invalid_arg(lib, call, name):
    assert call(lib, row_w=None) == -1
    msg = lib.mas_last_error().decode()
    assert msg.startswith(name + ':') and 'row_w' in msg
    assert call(lib, row_w=P + 2) == -1
    assert 'row_w' in lib.mas_last_error().decode()


@pytest.mark.parametrize('bad', [
    dict(packed=None), dict(x=None), dict(acts=None), dict(old_logp=None), dict(adv=None), dict(ret=None),
    dict(h1=None), dict(h2=None), dict(da1=None), dict(da2=None), dict(dz=None), dict(part=None),
    dict(obs_dim=0), dict(n_rows=0), dict(n_rows=-4), dict(ld=510),
    dict(x_stride=156), dict(x=P + 8),
])
def test_train_w_refuses_what_train_ld_refuses(lib, bad):
    assert _train_w(lib, **bad) == -1
    assert lib.mas_last_error().decode().startswith('mas_policy_train_w:')


@pytest.mark.parametrize('bad', [
    dict(packed=None), dict(x=None), dict(acts=None), dict(old_logp=None), dict(adv=None), dict(ret=None),
    dict(h1=None), dict(da1=None), dict(da2=None), dict(part=None), dict(out=None), dict(scratch=None),
    dict(obs_dim=0), dict(n_rows=0), dict(ld=510), dict(x_stride=156), dict(x=P + 8),
])
def test_train_dw3_w_refuses_what_train_dw3_refuses(lib, bad):
    assert _train_dw3_w(lib, **bad) == -1
    assert lib.mas_last_error().decode().startswith('mas_policy_train_dw3_w:')


@pytest.mark.parametrize('kw', [dict(n_rows=512 + 32, ld=640), dict(obs_dim=468, x_stride=480), dict(ld=577)])
def test_train_dw3_w_is_unsupported_where_train_dw3_is(lib, kw):
    # a partial 256-row block, a run-time layer-1 depth, an odd ld: refused before any launch
    assert _train_dw3_w(lib, **kw) == abi.MAS_ERR_UNSUPPORTED
    assert lib.mas_last_error().decode().startswith('mas_policy_train_dw3_w:')


def test_alive_refuses_a_null_handle(lib):
    assert lib.mas_alive(None, ctypes.c_void_p(P), None) == -1
    assert lib.mas_last_error().decode().startswith('mas_alive:')
