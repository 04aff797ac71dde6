"""The argument checks of mas_ret_stats, mas_ret_stats_scratch_doubles and
mas_gae_scaled come before any HIP call: they run here without a GPU, on null
or never-dereferenced device pointers.  (Every accepted call ends in a launch,
so only the refusals are exercised.)"""
import ctypes
import math

import pytest

from masurvival import abi

P = [4096 * (k + 1) for k in range(8)]  # distinct, 16-B aligned, never dereferenced addresses
RET_POINTERS = ('rewards', 'done', 'ret_carry', 'sums', 'scratch')
GAE_POINTERS = ('rewards', 'values', 'done', 'reward_scale', 'advantages', 'returns', 'adv_sums', 'scratch')
NAMES = ('mas_ret_stats_scratch_doubles', 'mas_ret_stats', 'mas_gae_scaled')


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _v(p):
    return ctypes.c_void_p(p)


def _ret(lib, T=16, n_columns=1024, n_agents=4, gamma=0.99, **ptr):
    p = dict(zip(RET_POINTERS, P))
    p.update(ptr)
    return lib.mas_ret_stats(T, n_columns, n_agents, _v(p['rewards']), _v(p['done']), gamma, _v(p['ret_carry']),
                             _v(p['sums']), _v(p['scratch']), None)


def _gae(lib, T=16, n_columns=1024, n_agents=4, gamma=0.99, lam=0.95, reward_clip=10.0, **ptr):
    p = dict(zip(GAE_POINTERS, P))
    p.update(ptr)
    return lib.mas_gae_scaled(T, n_columns, n_agents, _v(p['rewards']), _v(p['values']), _v(p['done']), gamma, lam,
                              _v(p['reward_scale']), reward_clip, _v(p['advantages']), _v(p['returns']),
                              _v(p['adv_sums']), _v(p['scratch']), None)


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


SHAPE_REFUSALS = [
    (dict(T=0), 'T > 0'),
    (dict(T=-1), 'T > 0'),
    (dict(n_columns=0), 'n_columns'),
    (dict(n_columns=-4), 'n_columns'),
    (dict(n_agents=0), 'n_agents'),
    (dict(n_agents=-1), 'n_agents'),
    (dict(n_columns=1025, n_agents=4), 'multiple'),
    (dict(n_columns=3, n_agents=4), 'multiple'),
]


@pytest.mark.parametrize('kw,word', SHAPE_REFUSALS + [({name: None}, 'null') for name in RET_POINTERS] + [
    (dict(n_columns=1 << 39, n_agents=1), 'too large'),          # 2^31 workgroups of 256 columns
    (dict(n_columns=(1 << 39) + 4, n_agents=4), 'too large'),
    (dict(n_columns=1 << 39, n_agents=1, scratch=None), 'null'),  # the pointers are looked at first
    (dict(gamma=math.nan), 'gamma'),
    (dict(gamma=math.inf), 'gamma'),
    (dict(gamma=-math.inf), 'gamma'),
    (dict(gamma=math.nan, T=0), 'T > 0'),                         # the shape first
])
def test_ret_stats_refusals(lib, kw, word):
    _invalid(lib, _ret, 'mas_ret_stats', word, **kw)


def test_ret_stats_scratch_doubles(lib):
    f = lib.mas_ret_stats_scratch_doubles
    assert f(0) == -1 and f(-1) == -1 and f(-(1 << 40)) == -1
    for n in (1, 2, 255, 256, 257, 511, 512, 513, 1025, 65536, 65537, 1 << 20, (1 << 39) - 1):
        assert f(n) == 2 * ((n + 255) // 256), n
        assert f(n) <= lib.mas_gae_scratch_doubles(n)  # a GAE scratch of the same columns serves both calls


@pytest.mark.parametrize('kw,word', SHAPE_REFUSALS + [({name: None}, 'null') for name in GAE_POINTERS] + [
    (dict(n_columns=1 << 37, n_agents=1), 'too large'),          # 2^31 workgroups of 64 columns, as mas_gae
    (dict(n_columns=1 << 37, n_agents=1, reward_scale=None), 'null'),
    (dict(reward_clip=0.0), 'reward_clip'),
    (dict(reward_clip=-0.0), 'reward_clip'),
    (dict(reward_clip=-1.0), 'reward_clip'),
    (dict(reward_clip=-math.inf), 'reward_clip'),
    (dict(reward_clip=math.nan), 'reward_clip'),
    (dict(reward_clip=math.nan, values=None), 'null'),            # the pointers first
])
def test_gae_scaled_refusals(lib, kw, word):
    _invalid(lib, _gae, 'mas_gae_scaled', word, **kw)


@pytest.mark.parametrize('scan', ['0', '1'])
def test_gae_scaled_refusals_do_not_depend_on_the_form(lib, scan, monkeypatch):
    monkeypatch.setenv('MAS_GAE_SCAN', scan)
    _invalid(lib, _gae, 'mas_gae_scaled', 'reward_clip', reward_clip=0.0)
    _invalid(lib, _gae, 'mas_gae_scaled', 'too large', n_columns=1 << 37, n_agents=1)


def test_python_wrappers_refuse_host_tensors_before_the_library():
    torch = pytest.importorskip('torch')
    from masurvival.ppo import ret_stats
    r = torch.zeros((4, 6))
    d = torch.zeros((4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ret_stats(r, d, 0.99, torch.zeros(6), torch.zeros(2, dtype=torch.float64), 3)
