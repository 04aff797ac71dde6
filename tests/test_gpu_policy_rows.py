"""Every row of what the PPO train kernels store (mas_policy_train_ld and
mas_policy_train_rm: k_policy_train in its 32-bit offset, 64-bit offset and
row-major forms, k_policy_train_cw, k_policy_train_db) against the staged
fp64 reference of tests/policy_rows_ref.py: h1, h2, dz, dA2, dA1 per element
within about one bf16 rounding, the loss partials, the clipped count exactly,
and nothing written outside the rows.  The bounds and what they reject are
stated in policy_rows_ref.py and checked by test_policy_rows_reference.py;
the figures measured on the MI355X are in profiles/train_rows_check.txt (worst
|d| / bound 0.994, dA2 of the grid-stride case; the fp32 constant as it stands).

The kernels are called through ctypes on buffers the test owns, the kernel
chosen by the per-call environment switches; the shapes are the smallest that
reach each path of policy_train's dispatch (csrc/mas_policy.hip).

Also here: the layer-3 gradient of the fused kernel (mas_policy_train_dw3) at
non-default loss coefficients, and the act kernel's log-prob and value against
the train kernel's on the same rows."""
import ctypes

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import policy_rows_ref as R  # noqa: E402
from masurvival import ppo as ppo_mod  # noqa: E402
from masurvival.abi import check  # noqa: E402
from masurvival.ppo import FusedPolicy, PPOConfig  # noqa: E402

SENTINEL = -1234.0  # no activation or gradient here comes near it
RM_LDH = 264        # row stride of the row-major h1 / h2: >= 257, a multiple of 8
RM_PAD_ROWS = 4     # rows allocated past M in the row-major buffers

# path -> environment switches (None: unset); 'rm' calls mas_policy_train_rm, the others mas_policy_train_ld
PATHS = {
    'db': dict(MAS_POL_DB=None, MAS_POL_CW=None, MAS_POL_FORCE_OFF64=None),
    'cw': dict(MAS_POL_DB='0', MAS_POL_CW=None, MAS_POL_FORCE_OFF64=None),
    'plain': dict(MAS_POL_DB='0', MAS_POL_CW='0', MAS_POL_FORCE_OFF64=None),
    'off64': dict(MAS_POL_DB=None, MAS_POL_CW=None, MAS_POL_FORCE_OFF64='1'),
    'rm': dict(MAS_POL_DB=None, MAS_POL_CW=None, MAS_POL_FORCE_OFF64=None),
}


def _grid_stride_rows():
    return 256 * (torch.cuda.get_device_properties(0).multi_processor_count + 3)


# (path, D, M, policy kind, coefficient set); M = 0: the grid-stride size
CASES = [
    # k_policy_train_db<10> + the partial last block on k_policy_train; db<9> on two blocks; grid-stride
    ('db', 160, 326, 'plain', 'A'), ('db', 138, 512, 'plain', 'A'), ('db', 160, 0, 'plain', 'A'),
    # k_policy_train_cw<10> and <0>
    ('cw', 160, 326, 'plain', 'A'), ('cw', 468, 130, 'plain', 'A'),
    # k_policy_train<10 / 9 / 0>: pair stores (M and ld even), scalar stores (odd M)
    ('plain', 160, 326, 'plain', 'A'), ('plain', 138, 326, 'plain', 'A'), ('plain', 468, 130, 'plain', 'A'),
    ('plain', 160, 77, 'plain', 'A'), ('plain', 138, 1, 'plain', 'A'),
    # 64-bit store offsets
    ('off64', 160, 326, 'plain', 'A'), ('off64', 160, 77, 'plain', 'A'),
    # row-major
    ('rm', 160, 326, 'plain', 'A'), ('rm', 138, 77, 'plain', 'A'),
    # the other coefficient sets, once per kernel body
    ('db', 160, 326, 'plain', 'B'), ('db', 160, 326, 'plain', 'C'),
    ('cw', 160, 326, 'plain', 'B'), ('cw', 160, 326, 'plain', 'C'),
    ('plain', 160, 326, 'plain', 'B'), ('plain', 160, 326, 'plain', 'C'),
    ('rm', 160, 326, 'plain', 'B'), ('rm', 160, 326, 'plain', 'C'),
    # saturated tanh and peaked heads; zero weights (z = the biases)
    ('db', 160, 326, 'x4', 'A'), ('plain', 160, 326, 'x4', 'A'),
    ('db', 160, 326, 'zero', 'A'), ('plain', 160, 326, 'zero', 'A'),
]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _setenv(monkeypatch, path):
    for k, v in PATHS[path].items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _policy(D, kind, rm=False, monkeypatch=None):
    p = R.make_policy(D, kind).cuda()
    if rm:
        monkeypatch.setattr(ppo_mod, '_POL_LAYOUT', 'rm')  # FusedPolicy then builds _rm_q
    fp = FusedPolicy(p, D, torch.device('cuda'))
    fp.pack()
    return p, fp


def _rows(fp, D, M, seed=7):
    """(x_buffer rows with random bf16 values, the generator that drew them)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    xb = fp.x_buffer(M)
    xb[:, :D] = (torch.randn((M, D), device='cuda', generator=g) * 2.0).bfloat16()
    return xb, g


class Buffers:
    """The activation buffers of one call, sentinel-filled: feature-major
    [257 | 256 | 16][ld] with ld = M + 64 (+ 1 for odd M), or row-major
    [M + RM_PAD_ROWS][RM_LDH | 256 | 16]; partials with one record to spare."""

    def __init__(self, lib, M, rm):
        self.M, self.rm = M, rm
        bf = dict(dtype=torch.bfloat16, device='cuda')
        self.nb = int(lib.mas_policy_blocks(M))
        self.part = torch.full((self.nb + 1, 4), float('nan'), device='cuda')
        self.part[self.nb] = SENTINEL
        if rm:
            rows = M + RM_PAD_ROWS
            shapes = dict(h1=(rows, RM_LDH), h2=(rows, RM_LDH), da1=(rows, 256), da2=(rows, 256), dz=(rows, 16))
        else:
            self.ld = ld = M + 64 + (M & 1)
            shapes = dict(h1=(257, ld), h2=(257, ld), da1=(256, ld), da2=(256, ld), dz=(16, ld))
        self.t = {k: torch.full(s, SENTINEL, **bf) for k, s in shapes.items()}

    def refill(self):
        for t in self.t.values():
            t.fill_(SENTINEL)
        self.part.fill_(float('nan'))
        self.part[self.nb] = SENTINEL

    def run(self, fp, xb, batch, cf):
        acts, old_logp, adv, ret = batch
        clip, vf, ec, sc = cf
        t, M = self.t, self.M
        head = (_ptr(fp.packed), fp.D, M, _ptr(xb), fp.Dx, _ptr(acts), _ptr(old_logp), _ptr(adv), _ptr(ret),
                clip, vf, ec, sc)
        if self.rm:
            check(fp.lib.mas_policy_train_rm(*head, _ptr(t['h1']), _ptr(t['h2']), RM_LDH, _ptr(t['da1']),
                                             _ptr(t['da2']), _ptr(t['dz']), _ptr(self.part), None))
        else:
            check(fp.lib.mas_policy_train_ld(*head, _ptr(t['h1']), _ptr(t['h2']), _ptr(t['da1']), _ptr(t['da2']),
                                             _ptr(t['dz']), self.ld, _ptr(self.part), None))
        torch.cuda.synchronize()

    def outputs(self, fp):
        """The stored tensors as [M, F] in natural feature order, and partials.sum(0)."""
        t, M = self.t, self.M
        if self.rm:
            q = fp._rm_q  # feature -> stored column
            out = {k: t[k][:M, :256].index_select(1, q) for k in ('h1', 'h2', 'da1', 'da2')}
            out['dz'] = t['dz'][:M]
        else:
            out = {k: t[k][:256, :M].T for k in ('h1', 'h2', 'da1', 'da2')}
            out['dz'] = t['dz'][:, :M].T
        out = {k: v.float() for k, v in out.items()}
        out['partials'] = self.part[:self.nb].double().sum(0)
        return out

    def untouched(self):
        """Names of the regions outside the rows that no longer hold the sentinel."""
        t, M, bad = self.t, self.M, []
        s = torch.tensor(SENTINEL, dtype=torch.bfloat16, device='cuda')
        for k, v in t.items():
            if self.rm:
                if not bool((v[M:] == s).all()):
                    bad.append(k + ' rows past M')
                if k in ('h1', 'h2') and not bool((v[:, 256:] == s).all()):
                    bad.append(k + ' columns [256, ld): the ones column and the padding')
            else:
                if not bool((v[:, M:] == s).all()):
                    bad.append(k + ' columns [M, ld)')
                if k in ('h1', 'h2') and not bool((v[256] == s).all()):
                    bad.append(k + ' row 256')
        if not bool((self.part[self.nb] == SENTINEL).all()):
            bad.append('partials past the last block')
        return bad


@pytest.mark.parametrize('path,D,M,kind,cset', CASES)
def test_train_rows_match_fp64_reference(path, D, M, kind, cset, monkeypatch):
    M = M or _grid_stride_rows()
    rm = path == 'rm'
    _setenv(monkeypatch, path)
    p, fp = _policy(D, kind, rm, monkeypatch)
    P = R.params(p)
    xb, g = _rows(fp, D, M)
    x = xb[:, :D]
    cf = R.coef(cset, M)
    B = Buffers(fp.lib, M, rm)
    # h2 does not depend on the batch: a first call on a null batch yields the
    # kernel's own, from which make_batch places every ratio (policy_rows_ref.make_batch)
    null = (torch.zeros((M, 6), dtype=torch.int8, device='cuda'),) + tuple(torch.zeros(M, device='cuda')
                                                                            for _ in range(3))
    B.run(fp, xb, null, cf)
    batch = R.make_batch(P, x, cf, g, h2=B.outputs(fp)['h2'])
    B.refill()
    B.run(fp, xb, batch, cf)
    out = B.outputs(fp)
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    res = R.check_rows(P, x, batch, cf, out)
    print(f'{path} D={D} M={M} {kind} {cset}: ' + ' '.join(f'{k} {res[k]:.3f}' for k in R.STAGES)
          + f' clipped {res["clipped"]:+.0f} near_clip {res["near_clip"]}')
    assert res['near_clip'] == 0, res
    for k in R.STAGES:
        assert res[k] <= 1.0, (k, res)
    assert res['clipped'] == 0.0, res
    assert B.untouched() == []


@pytest.mark.parametrize('cset', ['B', 'C'])
def test_fused_layer3_gradient_at_other_coefficients(cset, monkeypatch):
    """FusedPolicy.grads on the fused path (mas_policy_train_dw3, which stores
    neither h2 nor dz) at (160, 512) with the clip, vf_coef and ent_coef of
    coefficient sets B and C (grads always passes scale = 1 / M): head.weight
    and head.bias gradients against dz^T h2 and the column sums of dz of the
    unforced fp64 chain, within the per-row bounds summed over the rows
    (policy_rows_ref.check_dw3)."""
    D, M = 160, 512
    for k in ('MAS_POL_DB', 'MAS_POL_CW', 'MAS_POL_FORCE_OFF64', 'MAS_POL_DW3'):
        monkeypatch.delenv(k, raising=False)
    assert ppo_mod._POL_LAYOUT == 'fm' and '3' in ppo_mod._DW_LAYERS
    p, fp = _policy(D, 'plain')
    P = R.params(p)
    xb, g = _rows(fp, D, M)
    x = xb[:, :D]
    clip, vf, ec, _ = R.COEF[cset]
    cf = (clip, vf, ec, 1.0 / M)
    batch = R.make_batch(P, x, cf, g)
    fp.grads(xb, *batch, PPOConfig(clip=clip, vf_coef=vf, ent_coef=ec))
    torch.cuda.synchronize()
    assert 'h2' not in fp._bufs, 'the call stored h2 / dz: it took the unfused path'
    res = R.check_dw3(P, x, batch, cf, p.head.weight.grad, p.head.bias.grad)
    print(f'fused dW3 {cset}: dw3 {res["dw3"]:.3f} db3 {res["db3"]:.3f}')
    assert res['dw3'] <= 1.0 and res['db3'] <= 1.0, res


@pytest.mark.parametrize('D,M', [(160, 326), (138, 77)])
def test_act_and_train_agree_on_logp_and_value(D, M, monkeypatch):
    """old_logp = the act kernel's own logp of the actions it drew, adv = 1,
    ret = the act kernel's value, same packed policy.  The two kernels compute
    the log-prob and the value bit for bit alike (measured on the MI355X:
    both differences exactly 0), so the train kernel's ratio is exactly 1 on
    every row: no row clipped, sum(pg) = -M and sum((v - ret)^2) = 0, all
    exact (the issue's bounds, 1e-4 and 1e-8 on the means, tightened to
    equality)."""
    _setenv(monkeypatch, 'db')
    p, fp = _policy(D, 'plain')
    xb, g = _rows(fp, D, M)
    acts = torch.empty((M, 6), dtype=torch.int8, device='cuda')
    lp = torch.empty((M,), device='cuda')
    v = torch.empty((M,), device='cuda')
    fp.act_x(xb, 3, 5, acts, lp, v)
    B = Buffers(fp.lib, M, False)
    B.run(fp, xb, (acts, lp, torch.ones(M, device='cuda'), v), R.coef('A', M))
    part = B.outputs(fp)['partials']
    pg, vl, clipped = float(part[0]), float(part[1]), float(part[3])
    print(f'act/train D={D} M={M}: |sum pg / M + 1| = {abs(pg / M + 1.0):.3g}, sum (v - ret)^2 / M = {vl / M:.3g}, '
          f'clipped {clipped:.0f}')
    assert clipped == 0.0
    assert pg == -float(M)
    assert vl == 0.0
    assert B.untouched() == []
