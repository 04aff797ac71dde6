"""mas_policy_act_sel's argument checks come before any HIP call: they run
here without a GPU, on null or never-dereferenced device pointers."""
import ctypes

import pytest

from masurvival import abi


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def _call(lib, n_envs, n_agents, mask, ptr=None, x_stride=160, packed=None):
    p = ctypes.c_void_p(ptr)
    return lib.mas_policy_act_sel(ctypes.c_void_p(packed if packed is not None else ptr), 160, n_envs, n_agents, mask,
                                  0, p, x_stride, 1, 2, 0, p, p, p, None, None)


def test_symbol_is_declared_optional_and_present(lib):
    assert 'mas_policy_act_sel' in abi.SIGNATURES and 'mas_policy_act_sel' in abi.OPTIONAL
    assert hasattr(lib, 'mas_policy_act_sel')
    assert lib.mas_abi_version() == 3


@pytest.mark.parametrize('n_agents,mask,word', [
    (4, 0, 'agent_mask'),          # a zero mask
    (4, 0b10000, 'agent_mask'),    # a bit at n_agents
    (0, 0b1, 'n_agents'),
    (33, 0b1, 'n_agents'),
])
def test_bad_mask_or_agent_count_is_invalid_arg(lib, n_agents, mask, word):
    assert _call(lib, 8, n_agents, mask) == -1
    msg = lib.mas_last_error().decode()
    assert msg.startswith('mas_policy_act_sel') and word in msg


def test_full_32_agent_mask_is_accepted(lib):
    # the checks pass and nothing is launched for zero envs
    assert _call(lib, 0, 32, 0xFFFFFFFF, ptr=4096) == 0


def test_other_invalid_arguments(lib):
    assert _call(lib, -1, 4, 0b11, ptr=4096) == -1          # n_envs < 0
    assert _call(lib, 8, 4, 0b11, ptr=None) == -1           # null pointers
    assert 'null' in lib.mas_last_error().decode()
    assert _call(lib, 8, 4, 0b11, ptr=4096, packed=0) == -1  # null packed alone
    assert _call(lib, 8, 4, 0b11, ptr=4096, x_stride=156) == -1  # a stride act_x refuses
    assert _call(lib, 8, 4, 0b11, ptr=4096 + 8) == -1       # x not 16-B aligned


def test_zero_envs_is_ok_without_a_launch(lib):
    assert _call(lib, 0, 4, 0b0011, ptr=4096) == 0
