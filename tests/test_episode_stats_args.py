"""The argument checks of mas_episode_stats and
mas_episode_stats_scratch_doubles come before any HIP call: they run here
without a GPU, on null or never-dereferenced device pointers.  (Every accepted
call ends in a launch, so only the refusals are exercised.)"""
import ctypes

import pytest

from masurvival import abi
from masurvival.ppo import EPISODE_STATS_CHUNK, episode_stats_geometry

P = [4096 * (k + 1) for k in range(6)]  # distinct, aligned, never dereferenced addresses
POINTERS = ('rewards', 'done', 'ret_carry', 'len_carry', 'record', 'scratch')
NAMES = ('mas_episode_stats_scratch_doubles', 'mas_episode_stats')
WG, MAX_AGENTS = episode_stats_geometry()  # of the loaded library: the tests hold for any build of it
I64_MAX = (1 << 63) - 1


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _call(lib, T=16, n_envs=1024, n_agents=4, side_mask=0b0011, **ptr):
    p = dict(zip(POINTERS, P))
    p.update(ptr)
    return lib.mas_episode_stats(T, n_envs, n_agents, side_mask, *[ctypes.c_void_p(p[k]) for k in POINTERS], None)


def test_symbols_are_declared_optional_and_present(lib):
    for name in NAMES:
        assert name in abi.SIGNATURES and name in abi.OPTIONAL, name
        assert hasattr(lib, name), name
    assert lib.mas_abi_version() == 3
    assert WG % 64 == 0 and 64 <= WG <= 1024 and EPISODE_STATS_CHUNK >= 2 and MAX_AGENTS == 8


@pytest.mark.parametrize('kw,word', [
    (dict(T=0), 'T > 0'),
    (dict(T=-1), 'T > 0'),
    (dict(n_envs=0), 'n_envs'),
    (dict(n_envs=-4), 'n_envs'),
    (dict(n_agents=0, side_mask=0), 'n_agents'),
    (dict(n_agents=-1, side_mask=0), 'n_agents'),
    (dict(side_mask=0b10000), 'side_mask'),
    (dict(side_mask=1 << 31), 'side_mask'),
    (dict(n_agents=1, side_mask=0b10), 'side_mask'),
    (dict(n_agents=9, side_mask=1 << 9), 'side_mask'),            # refused as an argument before the agent limit
] + [({name: None}, 'null') for name in POINTERS] + [
    (dict(n_envs=WG << 31), 'too large'),                         # 2^31 workgroups
    (dict(n_envs=(WG << 31) + 1), 'too large'),
    (dict(n_envs=I64_MAX), 'too large'),                          # no overflow on the way to the block count
    (dict(n_envs=I64_MAX - WG + 2), 'too large'),
    (dict(n_envs=WG << 31, scratch=None), 'null'),                # the pointers are looked at first
    (dict(T=0, rewards=None), 'T > 0'),                           # the shape before the pointers
    (dict(side_mask=0b10000, done=None), 'side_mask'),
    (dict(n_agents=9, record=None), 'null'),                      # every refusal before the agent limit
    (dict(n_agents=9, n_envs=WG << 31), 'too large'),
])
def test_refusals(lib, kw, word):
    assert _call(lib, **kw) == -1, kw
    msg = lib.mas_last_error().decode()
    assert msg.startswith('mas_episode_stats:'), msg
    assert word in msg, msg


@pytest.mark.parametrize('n_agents,side_mask', [(9, 0), (9, 0b111), (16, 0xFF), (32, 0xFFFF0000), (33, 1), (1000, 0)])
def test_more_agents_than_the_kernel_takes_is_unsupported(lib, n_agents, side_mask):
    assert _call(lib, n_agents=n_agents, side_mask=side_mask) == abi.MAS_ERR_UNSUPPORTED
    msg = lib.mas_last_error().decode()
    assert msg.startswith('mas_episode_stats:') and 'n_agents' in msg, msg


def test_the_largest_grid_that_fits_is_not_refused_for_its_size(lib):
    # one env fewer than 'too large', with a null pointer so that nothing is launched
    assert _call(lib, n_envs=(WG << 31) - WG, scratch=None) == -1
    assert 'null' in lib.mas_last_error().decode()


def test_scratch_doubles(lib):
    f = lib.mas_episode_stats_scratch_doubles
    for n_envs, n_agents in ((0, 4), (-1, 4), (-(1 << 40), 1), (64, 0), (64, -1), (64, MAX_AGENTS + 1), (64, 32),
                             (64, 33), (WG << 31, 4), (1 << 62, 8), (I64_MAX, 1), (I64_MAX - 1, 8)):
        assert f(n_envs, n_agents) == -1, (n_envs, n_agents)
    for n in (1, 2, WG - 1, WG, WG + 1, 2 * WG - 1, 2 * WG, 2 * WG + 1, 1025, 65536, 65537, 257 * WG + 1, 1 << 20,
              (WG << 31) - WG):
        for a in range(1, MAX_AGENTS + 1):
            assert f(n, a) == (6 + 2 * a) * ((n + WG - 1) // WG), (n, a)


def test_python_wrapper_refuses_host_tensors_before_the_library():
    torch = pytest.importorskip('torch')
    from masurvival.ppo import episode_stats
    r = torch.zeros((4, 6))
    d = torch.zeros((4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError):
        episode_stats(r, d, 3, torch.zeros(6, dtype=torch.float64), torch.zeros(2, dtype=torch.int32),
                      torch.zeros(12, dtype=torch.float64))
    with pytest.raises(ValueError):
        episode_stats(r, d, 3, torch.zeros(6, dtype=torch.float64), torch.zeros(2, dtype=torch.int32),
                      torch.zeros(12, dtype=torch.float64), side_mask=0b1000)
