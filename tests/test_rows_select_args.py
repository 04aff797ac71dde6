"""mas_rows_select's argument checks come before any HIP call: they run here
without a GPU, on null or never-dereferenced device pointers."""
import ctypes

import pytest

from masurvival import abi

P, Q = 4096, 8192  # two distinct, 16-B aligned, never dereferenced addresses


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _arr(*ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _call(lib, n_envs=8, n_agents=4, mask=0b0011, x=P, x_stride=176, x_out=Q, x_out_stride=176, x_cols=176,
          actions=P, actions_out=Q, n_f32=2, f_in=(P, P + 64), f_out=(Q, Q + 64)):
    v = ctypes.c_void_p
    return lib.mas_rows_select(n_envs, n_agents, mask, v(x), x_stride, v(x_out), x_out_stride, x_cols, v(actions),
                               v(actions_out), n_f32, _arr(*f_in), _arr(*f_out), None)


def _invalid(lib, word=None, **kw):
    assert _call(lib, **kw) == -1, kw
    msg = lib.mas_last_error().decode()
    assert msg.startswith('mas_rows_select'), msg
    if word is not None:
        assert word in msg, msg


def test_symbol_is_declared_optional_and_present(lib):
    assert 'mas_rows_select' in abi.SIGNATURES and 'mas_rows_select' in abi.OPTIONAL
    assert hasattr(lib, 'mas_rows_select')
    assert lib.mas_abi_version() == 3


@pytest.mark.parametrize('n_agents,mask,word', [
    (0, 0b1, 'n_agents'),
    (33, 0b1, 'n_agents'),
    (4, 0, 'agent_mask'),          # a zero mask
    (4, 0b10000, 'agent_mask'),    # a bit at n_agents
    (31, 0x80000000, 'agent_mask'),
])
def test_bad_mask_or_agent_count(lib, n_agents, mask, word):
    _invalid(lib, word, n_agents=n_agents, mask=mask)


def test_negative_n_envs(lib):
    _invalid(lib, 'n_envs', n_envs=-1)


@pytest.mark.parametrize('n_f32', [-1, 5])
def test_n_f32_outside_0_to_4(lib, n_f32):
    _invalid(lib, 'n_f32', n_f32=n_f32)


@pytest.mark.parametrize('kw', [
    dict(x=None), dict(x_out=None), dict(actions=None), dict(actions_out=None),
    dict(f_in=(P, None)), dict(f_out=(None, Q + 64)),
])
def test_half_null_pair(lib, kw):
    _invalid(lib, 'half-null', **kw)


@pytest.mark.parametrize('kw', [
    dict(x_cols=0), dict(x_cols=-8), dict(x_cols=172),   # not a positive multiple of 8
    dict(x_cols=184),                                    # larger than both strides
    dict(x_cols=176, x_stride=168),                      # larger than the input stride
    dict(x_cols=176, x_out_stride=168),                  # larger than the output stride
])
def test_bad_x_cols(lib, kw):
    _invalid(lib, 'x_cols', **kw)


@pytest.mark.parametrize('kw', [
    dict(x_stride=180), dict(x_out_stride=180),          # strides that are no multiple of 8
    dict(x=P + 8), dict(x_out=Q + 8),                    # x pointers not 16-B aligned
])
def test_bad_stride_or_alignment(lib, kw):
    _invalid(lib, None, **kw)


@pytest.mark.parametrize('kw', [
    dict(x_out=P), dict(actions_out=P), dict(f_out=(P, Q + 64)), dict(f_out=(Q, P + 64)),
])
def test_output_equal_to_its_input(lib, kw):
    _invalid(lib, 'equals its input', **kw)


def test_valid_arguments_with_zero_envs_launch_nothing(lib):
    assert _call(lib, n_envs=0) == 0
    # a full 32-agent mask
    assert _call(lib, n_envs=0, n_agents=32, mask=0xFFFFFFFF) == 0
    assert _call(lib, n_envs=0, n_agents=32, mask=0x80000001, n_f32=4, f_in=(P, P + 64, P + 128, P + 192),
                 f_out=(Q, Q + 64, Q + 128, Q + 192)) == 0


def test_every_pair_null_is_ok_without_a_launch(lib):
    assert _call(lib, n_envs=1000, x=None, x_out=None, actions=None, actions_out=None, n_f32=0, f_in=(),
                 f_out=()) == 0
    assert _call(lib, n_envs=1000, x=None, x_out=None, actions=None, actions_out=None, n_f32=2, f_in=(None, None),
                 f_out=(None, None)) == 0
