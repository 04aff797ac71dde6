"""The argument checks of mas_gae, mas_gae_scratch_doubles and
mas_adv_normalize come before any HIP call: they run here without a GPU, on
null or never-dereferenced device pointers.  (Every accepted call ends in a
launch, so only the refusals are exercised.)"""
import ctypes

import pytest

from masurvival import abi

P = [4096 * (k + 1) for k in range(7)]  # distinct, 16-B aligned, never dereferenced addresses
GAE_POINTERS = ('rewards', 'values', 'done', 'advantages', 'returns', 'adv_sums', 'scratch')


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _v(p):
    return ctypes.c_void_p(p)


def _gae(lib, T=16, n_columns=1024, n_agents=4, gamma=0.99, lam=0.95, **ptr):
    p = dict(zip(GAE_POINTERS, P))
    p.update(ptr)
    return lib.mas_gae(T, n_columns, n_agents, _v(p['rewards']), _v(p['values']), _v(p['done']), gamma, lam,
                       _v(p['advantages']), _v(p['returns']), _v(p['adv_sums']), _v(p['scratch']), None)


def _norm(lib, n=1024, adv=P[0], stats=P[1]):
    return lib.mas_adv_normalize(n, _v(adv), _v(stats), None)


def _invalid(lib, fn, name, word=None, **kw):
    assert fn(lib, **kw) == -1, kw
    msg = lib.mas_last_error().decode()
    assert msg.startswith(name + ':'), msg
    if word is not None:
        assert word in msg, msg


def test_symbols_are_declared_and_present(lib):
    for name in ('mas_gae', 'mas_gae_scratch_doubles', 'mas_adv_normalize'):
        assert name in abi.SIGNATURES and hasattr(lib, name), name


@pytest.mark.parametrize('kw,word', [
    (dict(T=0), 'T > 0'),
    (dict(T=-1), 'T > 0'),
    (dict(n_columns=0), 'n_columns'),
    (dict(n_columns=-4), 'n_columns'),
    (dict(n_agents=0), 'n_agents'),
    (dict(n_agents=-1), 'n_agents'),
    (dict(n_columns=1025, n_agents=4), 'multiple'),
    (dict(n_columns=3, n_agents=4), 'multiple'),
] + [({name: None}, 'null') for name in GAE_POINTERS] + [
    (dict(n_columns=1 << 37, n_agents=1), 'too large'),          # 2^31 workgroups of 64 columns
    (dict(n_columns=(1 << 37) + 4, n_agents=4), 'too large'),
    (dict(n_columns=1 << 37, n_agents=1, scratch=None), 'null'),  # the pointers are looked at first
])
def test_gae_refusals(lib, kw, word):
    _invalid(lib, _gae, 'mas_gae', word, **kw)


def test_gae_scratch_doubles(lib):
    f = lib.mas_gae_scratch_doubles
    assert f(0) == -1 and f(-1) == -1 and f(-(1 << 40)) == -1
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025, 65536, 65537, 1 << 20, (1 << 37) - 1):
        assert f(n) == 2 * ((n + 63) // 64), n


@pytest.mark.parametrize('kw,word', [
    (dict(n=0), 'n > 0'),
    (dict(n=-1), 'n > 0'),
    (dict(adv=None), 'null'),
    (dict(stats=None), 'null'),
    (dict(adv=P[0] + 4), '16-B'),
    (dict(adv=P[0] + 8), '16-B'),
    (dict(adv=P[0] + 1), '16-B'),
    (dict(n=1 << 41), 'too large'),            # 2^31 workgroups of 1024 elements
    (dict(n=(1 << 41) - 1023), 'too large'),
])
def test_adv_normalize_refusals(lib, kw, word):
    _invalid(lib, _norm, 'mas_adv_normalize', word, **kw)
