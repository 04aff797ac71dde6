"""The argument checks of mas_bot_act come before any HIP call: they run here
without a GPU, on never-dereferenced device pointers.  (Every accepted call
with n_envs > 0 ends in a launch, so only the refusals and n_envs == 0 are
exercised.)"""
import ctypes

import pytest

from masurvival import abi
from masurvival.config import C1_CONFIG, C3_CONFIG, ResolvedConfig

X, ACT = 4096, 8192  # distinct, aligned, never dereferenced addresses
ROWS_PER_BLOCK = 32  # csrc/mas_bot.hip: 256 threads, 8 lanes per row
I64_MAX = (1 << 63) - 1


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _cfg(**fields):
    cs = ResolvedConfig(C3_CONFIG).to_struct()  # 2v2 with teams: obs_dim 160
    for k, v in fields.items():
        setattr(cs, k, v)
    return cs


def _call(lib, cfg='default', kind=1, n_envs=64, mask=0b1100, x=X, stride=176, actions=ACT):
    cs = _cfg() if cfg == 'default' else cfg
    return lib.mas_bot_act(ctypes.byref(cs) if cs is not None else None, kind, n_envs, mask,
                           ctypes.c_void_p(x) if x else None, stride, ctypes.c_void_p(actions) if actions else None,
                           None)


def test_symbol_is_declared_optional_and_present(lib):
    assert 'mas_bot_act' in abi.SIGNATURES and 'mas_bot_act' in abi.OPTIONAL
    assert hasattr(lib, 'mas_bot_act')
    assert lib.mas_abi_version() == 3
    from masurvival.bots import BOT_KINDS
    assert BOT_KINDS == {'idle': 0, 'hunter': 1, 'forager': 2}


@pytest.mark.parametrize('kw,word', [
    (dict(cfg=None), 'null cfg'),
    (dict(cfg=_cfg(n_agents=1)), 'config'),
    (dict(cfg=_cfg(n_heals=-1)), 'config'),
    (dict(cfg=_cfg(grid_size=17)), 'config'),          # > 256 cells
    (dict(cfg=_cfg(grid_size=2)), 'config'),           # too small for the spawns
    (dict(cfg=_cfg(zone_phases=0)), 'config'),
    (dict(cfg=_cfg(lidar_n_lasers=1)), 'config'),
    (dict(cfg=_cfg(n_agents=9, grid_size=8)), 'capacity class'),   # mas_create finds no class for it
    (dict(kind=-1), 'kind'),
    (dict(kind=3), 'kind'),
    (dict(mask=0), 'agent_mask'),
    (dict(mask=0b10000), 'agent_mask'),
    (dict(mask=1 << 31), 'agent_mask'),
    (dict(cfg=ResolvedConfig(C1_CONFIG).to_struct(), mask=0b100, stride=128), 'agent_mask'),
    (dict(n_envs=-1), 'n_envs'),
    (dict(n_envs=-(1 << 40)), 'n_envs'),
    (dict(n_envs=(ROWS_PER_BLOCK << 31) // 2, mask=0b0011), 'too large'),     # 2^31 blocks of two rows per env
    (dict(n_envs=ROWS_PER_BLOCK << 31, mask=0b0001), 'too large'),
    (dict(n_envs=I64_MAX), 'too large'),                                     # no overflow on the way
    (dict(n_envs=I64_MAX // 4 + 1, mask=0b1111), 'too large'),
    (dict(x=0), 'null'),
    (dict(actions=0), 'null'),
    (dict(stride=152), 'stride'),      # below obs_dim
    (dict(stride=180), 'stride'),      # no multiple of 8
    (dict(stride=0), 'stride'),
    (dict(stride=-176), 'stride'),
    (dict(x=X + 8), 'aligned'),        # x 16-B
    (dict(actions=ACT + 1), 'aligned'),  # actions 2-B
])
def test_refusals(lib, kw, word):
    assert _call(lib, **kw) == -1, kw
    msg = lib.mas_last_error().decode()
    assert msg.startswith('mas_bot_act:'), msg
    assert word in msg, msg


def test_the_checks_come_in_the_documented_order(lib):
    # a refused config before the kind, the kind before the mask, the size before the pointers
    assert _call(lib, cfg=_cfg(n_agents=1), kind=9) == -1 and 'config' in lib.mas_last_error().decode()
    assert _call(lib, kind=9, mask=0) == -1 and 'kind' in lib.mas_last_error().decode()
    assert _call(lib, n_envs=I64_MAX, x=0) == -1 and 'too large' in lib.mas_last_error().decode()


def test_the_largest_grid_that_fits_is_not_refused_for_its_size(lib):
    # one block fewer than 'too large', with a null pointer so that nothing is launched
    assert _call(lib, n_envs=(ROWS_PER_BLOCK << 31) - ROWS_PER_BLOCK - 1, mask=0b0001, x=0) == -1
    assert 'null' in lib.mas_last_error().decode()


def test_zero_envs_is_ok_and_launches_nothing(lib):
    for kind in (0, 1, 2):
        assert _call(lib, kind=kind, n_envs=0) == 0
    # ... but its arguments are still checked
    assert _call(lib, n_envs=0, mask=0) == -1
    assert _call(lib, n_envs=0, x=0) == -1


def test_the_smallest_valid_stride_is_obs_dim_rounded_to_16(lib):
    # 160 columns at 2v2: with no envs every check runs and nothing is launched
    assert _call(lib, stride=160, n_envs=0) == 0
    assert _call(lib, stride=144, n_envs=0) == -1 and 'stride' in lib.mas_last_error().decode()
    # 1v1 without teams: obs_dim 8 + 6 + 8 + 1 + 14 + 101 = 138 -> 144
    c1 = ResolvedConfig(C1_CONFIG).to_struct()
    assert _call(lib, cfg=c1, mask=0b01, stride=144, n_envs=0) == 0
    assert _call(lib, cfg=c1, mask=0b01, stride=136, n_envs=0) == -1


def test_python_wrapper_refuses_host_tensors_and_unknown_names():
    torch = pytest.importorskip('torch')
    from masurvival.bots import Bot, bot_act, parse_bot
    cs = _cfg()
    with pytest.raises(ValueError, match='device'):
        bot_act(cs, 'hunter', torch.zeros((8, 176), dtype=torch.bfloat16), 4, 0b11,
                torch.zeros((8, 6), dtype=torch.int8))
    for bad in ('bot:', 'bot:Hunter', 'bot:sniper', 'hunter', '', None, 3):
        with pytest.raises(ValueError):
            parse_bot(bad)
    assert parse_bot('bot:hunter') == Bot('hunter') and parse_bot(Bot('idle')).kind == 0
    assert parse_bot('bot:forager').kind == 2
