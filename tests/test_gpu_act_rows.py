"""Every row of what the act side draws -- mas_sample_actions (k_sample) on
the caller's logits, and the fused kernels mas_policy_act_rows (fp32 rows,
writing the bf16 rows), mas_policy_act_x and sampled mas_policy_act_sel, each
with the split sampler and with the one-half loop (MAS_ACT_SPLIT=0) -- against
the host restatement of the RNG stream in tests/sampler_ref.py: every head
whose two best fp64 scores are at least tau apart draws the reference's
option, a nearer head one of the reference's top two, every action is in
range, the log-prob is the fp64 log-softmax of the same logits within the
derived bound, the share of rows with a near head stays under 0.5 %, and
nothing is written past the rows.  tau and the bound are derived in
sampler_ref.py; what they reject is checked by test_sampler_reference.py.

The fused kernels' logits are mas_policy_act_sel's logits_out of the same rows
under the full mask.  All sixteen columns of it are held to the fp64 product
of the train kernel's stored h2 with W3, within policy_rows_ref's fp32 term.

The figures measured on the MI355X are in profiles/act_rows_check.txt."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import policy_rows_ref as R  # noqa: E402
import sampler_ref as S  # noqa: E402
import test_gpu_policy_rows as T  # noqa: E402
from masurvival.ppo import sample_actions_hip  # noqa: E402

DEV = 'cuda'
NAN_BITS = 0x7FC0BEEF  # a quiet NaN with a payload no kernel produces
ACT_SENTINEL = -7
PAD = 5                # rows allocated past M
BIG_SEED, BIG_STEP = 0xFEDCBA9876543210, (1 << 40) + 3
BIG_ROW = (1 << 33) + 5


class Out:
    """Sentinel-filled outputs of one call, PAD rows to spare."""

    def __init__(self, M, logits=False):
        n = M + PAD
        self.M = M
        self.a = torch.full((n, 6), ACT_SENTINEL, dtype=torch.int8, device=DEV)
        f = lambda *s: torch.full(s, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)  # noqa: E731
        self.lp, self.v = f(n), f(n)
        self.lg = f(n, 16) if logits else None

    def args(self):
        M = self.M
        return self.a[:M], self.lp[:M], self.v[:M]

    def untouched(self, rows=None):
        """Names of the outputs written outside `rows` (default: the first M)."""
        keep = torch.ones(self.a.shape[0], dtype=torch.bool, device=DEV)
        keep[:self.M] = False
        if rows is not None:
            keep[:self.M] = True
            keep[rows] = False
        bad = [] if bool((self.a[keep] == ACT_SENTINEL).all()) else ['actions']
        for k in ('lp', 'v', 'lg'):
            t = getattr(self, k)
            if t is not None and not bool((t.view(torch.int32)[keep] == NAN_BITS).all()):
                bad.append(k)
        return bad


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_draws(name, res):
    print(f'act_rows {name}: near_share {res["near_share"]:.5f} near_heads {res["near_heads"]} '
          f'runner_up {res["runner_up"]} runner_up_margin {res["runner_up_margin"]:.3g} logp {res["logp"]:.3f}')
    assert (res['wrong'], res['outside_top2'], res['range']) == (0, 0, 0), (name, res)
    assert res['near_share'] <= S.NEAR_CAP, (name, res)
    assert res['logp'] <= 1.0, (name, res)


# ---------------------------------------------------------------------------
# mas_sample_actions

def _sample_logits(M, stride, scale, seed=11):
    """Host logits [M, stride]: randn x scale in the 15 columns the kernel
    reads, NaN in the rest."""
    lg = np.full((M, stride), np.nan, dtype=np.float32)
    lg[:, :15] = (np.random.default_rng(seed + M).standard_normal((M, 15)) * scale).astype(np.float32)
    return lg


def _run_sample(lg, seed, step):
    M = lg.shape[0]
    out = Out(M)
    sample_actions_hip(torch.from_numpy(lg).to(DEV), seed, step, out.a[:M], out.lp[:M])
    torch.cuda.synchronize()
    assert out.untouched() == []
    assert bool((out.v.view(torch.int32) == NAN_BITS).all())  # the sampler has no value output
    return _np(out.a[:M]), _np(out.lp[:M])


@pytest.mark.parametrize('seed,step', [(1234, 7), (BIG_SEED, BIG_STEP)])
@pytest.mark.parametrize('scale', [0.0, 1.5, 6.0])
@pytest.mark.parametrize('stride', [16, 24])
@pytest.mark.parametrize('M', [1, 255, 256, 257, 4099])
def test_sample_actions_rows(M, stride, scale, seed, step):
    lg = _sample_logits(M, stride, scale)
    a, lp = _run_sample(lg, seed, step)
    _assert_draws(f'k_sample M={M} stride={stride} scale={scale} seed={seed:#x} step={step:#x}',
                  S.check_draws(lg, seed, step, 0, M, a, lp))


@pytest.mark.parametrize('kind', ['one', 'min', 'tie'])
def test_sample_actions_extreme_draw(kind):
    """The rows of sampler_ref.EXTREME: u = 1.0 wins against a logit of -30
    with a finite log-prob; u = 2^-25; two equal u on equal logits draw the
    lower index."""
    seed, step, row, h, k = S.EXTREME['sample'][kind]
    M = 4099
    lg = _sample_logits(M, 16, 0.0 if kind == 'tie' else 1.5)
    if kind == 'one':
        lg[row, S.HEAD_OFF[h] + k] = -30.0
    a, lp = _run_sample(lg, seed, step)
    res = S.check_draws(lg, seed, step, 0, M, a, lp)
    _assert_draws(f'k_sample extreme {kind}', res)
    assert np.isfinite(lp).all()
    if kind != 'min':
        assert int(a[row, h]) == k


# ---------------------------------------------------------------------------
# the fused kernels

def _obs(M, D, seed=7):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn((M, D), device=DEV, generator=g) * 2.0).contiguous()


def _xb(fp, M):
    """x_buffer rows with PAD rows past M that hold a sentinel."""
    xb = fp.x_buffer(M + PAD)
    xb[M:] = -1234.0
    return xb


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv('MAS_ACT_SPLIT', raising=False)
    else:
        monkeypatch.setenv('MAS_ACT_SPLIT', split)


def _reference_logits(fp, xb, M, A=1):
    """logits_out of act_sel under the full mask (seed and step do not enter)."""
    out = Out(M, logits=True)
    fp.act_sel(xb[:M], A, (1 << A) - 1, 0, 0, *out.args(), logits=out.lg[:M])
    torch.cuda.synchronize()
    assert out.untouched() == []
    return out.lg[:M]


def _check_fused(name, monkeypatch, fp, obs, M, seed, step, first_row, forced=None):
    """act (writing xb), act_x and sampled act_sel, each under MAS_ACT_SPLIT
    unset and =0, on the same rows.  forced: (row, head, option) to be drawn."""
    xb = _xb(fp, M)
    _set_split(monkeypatch, None)
    o = Out(M)
    fp.act(obs, seed, step, *o.args(), xb=xb[:M], first_row=first_row)
    torch.cuda.synchronize()
    assert bool((xb[M:] == -1234.0).all())
    lg_t = _reference_logits(fp, xb, M)
    lg = _np(lg_t)
    assert np.isfinite(lg).all()
    calls = {
        'act': lambda o: fp.act(obs, seed, step, *o.args(), xb=xb[:M], first_row=first_row),
        'act_x': lambda o: fp.act_x(xb[:M], seed, step, *o.args(), first_row=first_row),
        'act_sel': lambda o: fp.act_sel(xb[:M], 1, 1, seed, step, *o.args(), first_row=first_row),
    }
    for split in (None, '0'):
        _set_split(monkeypatch, split)
        for kname, call in calls.items():
            o = Out(M)
            call(o)
            torch.cuda.synchronize()
            a, lp = _np(o.a[:M]), _np(o.lp[:M])
            res = S.check_draws(lg, seed, step, first_row, M, a, lp)
            _assert_draws(f'{kname} split={split} {name}', res)
            assert torch.equal(_bits(o.v[:M]), _bits(lg_t[:, 15])), kname
            assert o.untouched() == [], kname
            if forced is not None:
                assert int(a[forced[0], forced[1]]) == forced[2], (kname, split)
    assert bool((xb[M:] == -1234.0).all())


DS = (160, 150, 144, 138, 468)   # KS = 10 full / partial k-step, KS = 9 full / partial, the chunked form
MS = (1, 31, 33, 133, 326)       # 133: one 128-row workgroup and 5 rows
FIRST_ROWS = (0, 77, BIG_ROW)

# (D, M, first_row, kind, seed, step): every D with every M, first_row in rotation;
# the other policy kinds; the large seed and step
FUSED = ([(D, M, FIRST_ROWS[(i + j) % 3], 'plain', 1234, 7) for i, D in enumerate(DS) for j, M in enumerate(MS)] +
         [(D, 133, 77, kind, 1234, 7) for kind in ('x4', 'zero') for D in (160, 150, 468)] +
         [(160, 326, BIG_ROW, 'plain', BIG_SEED, BIG_STEP), (144, 33, 77, 'x4', BIG_SEED, BIG_STEP),
          (468, 133, 0, 'zero', BIG_SEED, BIG_STEP)])


@pytest.mark.parametrize('D,M,first_row,kind,seed,step', FUSED)
def test_fused_act_rows(D, M, first_row, kind, seed, step, monkeypatch):
    p, fp = T._policy(D, kind)
    _check_fused(f'D={D} M={M} first_row={first_row:#x} {kind} seed={seed:#x} step={step:#x}', monkeypatch, fp,
                 _obs(M, D), M, seed, step, first_row)


@pytest.mark.parametrize('kind', ['one', 'min', 'tie'])
def test_fused_act_extreme_draw(kind, monkeypatch):
    """The rows of sampler_ref.EXTREME, reached through first_row.  'one' (u =
    1.0): the option is drawn by every kernel and the log-prob is finite (every
    case asserts a finite log-prob through the ratio).  'tie': a policy of zero
    parameters gives equal logits, and the two equal u draw the lower index."""
    seed, step, row, h, k = S.EXTREME['fused'][kind]
    D, M, at = 160, 33, 17
    p, fp = T._policy(D, 'plain')
    if kind == 'tie':
        with torch.no_grad():
            for q in p.parameters():
                q.zero_()
        fp.pack()
    _check_fused(f'extreme {kind}', monkeypatch, fp, _obs(M, D), M, seed, step, row - at,
                 forced=None if kind == 'min' else (at, h, k))


@pytest.mark.parametrize('D,A,N,mask', [(160, 3, 41, 0b101), (468, 8, 21, 0xA5)])
def test_act_sel_rows_under_a_noncontiguous_mask(D, A, N, mask, monkeypatch):
    _set_split(monkeypatch, None)
    seed, step, first_row = 1234, 7, 77
    M = N * A
    p, fp = T._policy(D, 'plain')
    xb, _ = T._rows(fp, D, M)
    lg = _reference_logits(fp, xb, M, A)
    agent = torch.arange(M, device=DEV) % A
    rows = torch.nonzero(((torch.full_like(agent, mask) >> agent) & 1).bool()).squeeze(1)
    o = Out(M, logits=True)
    fp.act_sel(xb, A, mask, seed, step, *o.args(), logits=o.lg[:M], first_row=first_row)
    torch.cuda.synchronize()
    assert o.untouched(rows) == []
    assert torch.equal(_bits(o.lg[rows]), _bits(lg[rows]))
    res = S.check_draws(_np(lg[rows]), seed, step, first_row, _np(rows), _np(o.a[rows]), _np(o.lp[rows]))
    _assert_draws(f'act_sel D={D} A={A} N={N} mask={mask:#x}', res)


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('split', [None, '0'])
def test_act_and_act_x_agree_bit_for_bit(D, split, monkeypatch):
    """act on fp32 rows, then act_x on the bf16 rows act wrote, at the same
    (seed, step, first_row): identical actions, log-probs and values."""
    _set_split(monkeypatch, split)
    M, seed, step, first_row = 133, BIG_SEED, BIG_STEP, BIG_ROW
    p, fp = T._policy(D, 'plain')
    obs = _obs(M, D)
    xb = _xb(fp, M)
    xb[:M, :fp.Dp] = 77.0  # the columns act has to write
    o1, o2 = Out(M), Out(M)
    fp.act(obs, seed, step, *o1.args(), xb=xb[:M], first_row=first_row)
    fp.act_x(xb[:M], seed, step, *o2.args(), first_row=first_row)
    torch.cuda.synchronize()
    # xb: the bf16 rounding of the rows, 1.0 in column D (act's own where D is inside the last
    # k-step, else x_buffer's), zeros in the other columns, the sentinel past M
    assert torch.equal(xb[:M, :D].view(torch.int16), obs.bfloat16().view(torch.int16))
    assert bool((xb[:M, D] == 1.0).all()) and bool((xb[:M, D + 1:] == 0.0).all())
    assert bool((xb[M:] == -1234.0).all())
    assert torch.equal(o1.a, o2.a)
    assert torch.equal(_bits(o1.lp), _bits(o2.lp)) and torch.equal(_bits(o1.v), _bits(o2.v))
    assert o1.untouched() == [] and o2.untouched() == []


@pytest.mark.parametrize('D', [160, 150, 138, 468])
def test_logits_out_all_columns_match_fp64(D, monkeypatch):
    """All sixteen columns of logits_out against fp64 h2_k W3^T + b3, h2_k the
    h2 the train kernel stores for the same rows (a call on a null batch),
    within policy_rows_ref's fp32 term FP32 (|h2_k| |W3|^T + |b3|) + 1e-6 per
    element: the act and the train kernel share h2 bit for bit, so no bf16
    rounding enters the bound."""
    M = 326
    T._setenv(monkeypatch, 'db')
    _set_split(monkeypatch, None)
    p, fp = T._policy(D, 'plain')
    P = R.params(p)
    xb, _ = T._rows(fp, D, M)
    B = T.Buffers(fp.lib, M, False)
    null = (torch.zeros((M, 6), dtype=torch.int8, device=DEV),) + tuple(torch.zeros(M, device=DEV) for _ in range(3))
    B.run(fp, xb, null, R.coef('A', M))
    h2 = B.outputs(fp)['h2'].double()
    assert B.untouched() == []
    lg = _reference_logits(fp, xb, M).double()
    ref = h2 @ P['W3'].T + P['b3']
    tol = R.FP32 * (h2.abs() @ P['W3'].abs().T + P['b3'].abs()) + 1e-6
    ratio = float(((lg - ref).abs() / tol).max())
    print(f'act_rows logits_out D={D} M={M}: worst |d| / bound {ratio:.3f}, max |d| {float((lg - ref).abs().max()):.3g}')
    assert ratio <= 1.0
