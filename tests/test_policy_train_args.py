"""The argument checks of the six PPO train entry points (mas_policy_train,
_ld, _dw3, _w, _dw3_w, _rm), one bad argument at a time: the return code and
the entry point's own name in front of mas_last_error().  Every check comes
before any HIP call, so the calls run here without a GPU on never-dereferenced
device pointers; no call in this file is a valid one."""
import ctypes

import pytest

from masurvival import abi

P = 4096  # a non-null, 16-B aligned "device pointer" that is never dereferenced
INVALID, UNSUPPORTED = -1, abi.MAS_ERR_UNSUPPORTED

HEAD = ['packed', 'obs_dim', 'n_rows', 'x', 'x_stride', 'acts', 'old_logp', 'adv', 'ret']
COEFS = ['clip', 'vf_coef', 'ent_coef', 'scale']
STORED = ['h1', 'h2', 'da1', 'da2', 'dz']
FUSED = ['h1', 'da1', 'da2', 'ld', 'part', 'out', 'scratch']
# entry point -> its parameters in call order (the stream, always null here, comes last)
FORMS = {
    'mas_policy_train': HEAD + COEFS + STORED + ['part'],
    'mas_policy_train_ld': HEAD + COEFS + STORED + ['ld', 'part'],
    'mas_policy_train_dw3': HEAD + COEFS + FUSED,
    'mas_policy_train_w': HEAD + ['row_w'] + COEFS + STORED + ['ld', 'part'],
    'mas_policy_train_dw3_w': HEAD + ['row_w'] + COEFS + FUSED,
    'mas_policy_train_rm': HEAD + COEFS + ['h1', 'h2', 'ld_h', 'da1', 'da2', 'dz', 'part'],
}
# a call every entry point would accept (never made as it stands)
GOOD = dict(obs_dim=160, n_rows=512, x_stride=176, clip=0.2, vf_coef=0.5, ent_coef=0.01, scale=1.0 / 512, ld=576,
            ld_h=264)
ACTIVATIONS = ('h1', 'h2', 'da1', 'da2', 'dz')


@pytest.fixture(scope='module')
def lib():
    return abi.load_library()


def call(lib, name, **bad):
    assert bad and set(bad) <= set(FORMS[name])
    args = []
    for prm in FORMS[name]:
        v = bad[prm] if prm in bad else GOOD.get(prm, P)
        args.append(v if prm in GOOD else ctypes.c_void_p(v))
    return getattr(lib, name)(*args, None)


def cases():
    out = []
    for name, prms in FORMS.items():
        def add(code, name=name, **bad):
            out.append(pytest.param(name, bad, code, id=name + ''.join(f'-{k}={v}' for k, v in bad.items())))

        for prm in prms:
            if prm not in GOOD and prm != 'row_w':
                add(INVALID, **{prm: None})
        add(INVALID, obs_dim=0)
        add(INVALID, n_rows=0)
        add(INVALID, n_rows=-4)
        if 'ld' in prms:
            add(INVALID, ld=510)
        add(INVALID, x_stride=156)
        add(INVALID, x=P + 8)
        if 'ld_h' in prms:
            add(INVALID, ld_h=256)
            add(INVALID, ld_h=260)
            for prm in ACTIVATIONS:
                add(INVALID, **{prm: P + 8})
        if 'out' in prms:
            # a partial 256-row block, a run-time layer-1 depth, an odd ld: refused before any launch
            add(UNSUPPORTED, n_rows=512 + 32, ld=640)
            add(UNSUPPORTED, obs_dim=468, x_stride=480)
            add(UNSUPPORTED, ld=577)
    return out


@pytest.mark.parametrize('name,bad,code', cases())
def test_one_bad_argument_is_refused_under_the_entry_points_name(lib, name, bad, code):
    assert call(lib, name, **bad) == code
    assert lib.mas_last_error().decode().startswith(name + ':')


@pytest.mark.parametrize('name', [n for n, prms in FORMS.items() if 'row_w' in prms])
@pytest.mark.parametrize('row_w', [None, P + 2])
def test_null_or_misaligned_row_w_is_invalid_arg(lib, name, row_w):
    assert call(lib, name, row_w=row_w) == INVALID
    msg = lib.mas_last_error().decode()
    assert msg.startswith(name + ':') and 'row_w' in msg


@pytest.mark.parametrize('name,fallback', [('mas_policy_train_dw3', 'mas_policy_train_ld'),
                                           ('mas_policy_train_dw3_w', 'mas_policy_train_w')])
def test_dw3_switched_off_per_call_is_unsupported_and_names_the_fallback(lib, monkeypatch, name, fallback):
    monkeypatch.setenv('MAS_POL_DW3', '0')
    getenv = ctypes.CDLL(None).getenv
    getenv.restype = ctypes.c_char_p
    assert getenv(b'MAS_POL_DW3') == b'0'  # the library's getenv sees it: the valid call below stops at the check
    # an argument that is bad either way still comes first ...
    assert call(lib, name, x=P + 8) == INVALID
    # ... and a shape that is unsupported either way is refused the same
    assert call(lib, name, ld=577) == UNSUPPORTED
    # the call that is valid without the switch: refused by it, nothing launched
    args = [GOOD[p] if p in GOOD else ctypes.c_void_p(P) for p in FORMS[name]]
    assert getattr(lib, name)(*args, None) == UNSUPPORTED
    msg = lib.mas_last_error().decode()
    assert msg.startswith(name + ':') and msg.rstrip().endswith(fallback)
