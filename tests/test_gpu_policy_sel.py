"""mas_policy_act_sel (FusedPolicy.act_sel): the act kernel over the agents a
bit mask selects, sampled or greedy, with the optional logits output.

The CPU tensors come from torch.manual_seed / CPU generators and are moved to
the device.  Bitwise comparisons go through view(int32): log-probs and values
are compared as bit patterns, and the float sentinel is a fixed NaN pattern."""
import copy

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.abi import MasError  # noqa: E402
from masurvival.ppo import HEADS, FusedPolicy, PolicyMLP  # noqa: E402

DEV = 'cuda'
NAN_BITS = 0x7FC0BEEF  # a quiet NaN with a payload no kernel produces
ACT_SENTINEL = -7


def _fused(D, seed):
    torch.manual_seed(seed)
    p = PolicyMLP(D, 256).to(DEV)
    fp = FusedPolicy(p, D, torch.device(DEV))
    fp.pack()
    return p, fp


def _rows(fp, M, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((M, fp.D), generator=g) * 3.0
    xb = fp.x_buffer(M)
    xb[:, :fp.D].copy_(obs.to(DEV))
    return xb


def _outputs(M, logits=False):
    a = torch.full((M, 6), ACT_SENTINEL, dtype=torch.int8, device=DEV)
    lp = torch.full((M,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    v = torch.full((M,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    lg = torch.full((M, 16), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32) if logits else None
    return a, lp, v, lg


def _bits(t):
    return t.view(torch.int32)


def _selected(M, A, mask):
    agent = torch.arange(M, device=DEV) % A
    return ((torch.full_like(agent, mask) >> agent) & 1).bool()


@pytest.mark.parametrize('D,A,N,masks,first_row', [
    (160, 4, 69, (0b0011, 0b1100), 0),      # four full waves and a tail of 10 logical rows
    (160, 4, 7, (0b0101, 0b1010), 0),       # non-contiguous mask, fewer than 32 rows
    (138, 3, 50, (0b001, 0b110), 3 * 77),   # odd agent count, KS = 9, shard offset
    (468, 8, 21, (0x0F, 0xF0), 0),          # the chunked KS = 0 form, 8 agents
    (160, 2, 33, (0b01, 0b10), 0),          # m = 1
    (160, 4, 40, (0b1111,), 1 << 20),       # full mask equals act_x
])
def test_union_of_masks_is_act_x_bit_for_bit(D, A, N, masks, first_row):
    _, fp = _fused(D, seed=D + A)
    M = N * A
    xb = _rows(fp, M, seed=N)
    xb0 = xb.clone()
    ra, rlp, rv, _ = _outputs(M)
    fp.act_x(xb, 5, 123, ra, rlp, rv, first_row=first_row)
    a, lp, v, lg = _outputs(M, logits=True)
    done = torch.zeros((M,), dtype=torch.bool, device=DEV)
    for mask in masks:
        fp.act_sel(xb, A, mask, 5, 123, a, lp, v, logits=lg, first_row=first_row)
        done |= _selected(M, A, mask)
        # rows of agents not selected so far still hold the sentinels
        assert bool((a[~done] == ACT_SENTINEL).all())
        for t in (lp, v):
            assert bool((_bits(t)[~done] == NAN_BITS).all())
        assert bool((_bits(lg)[~done] == NAN_BITS).all())
        # selected rows equal act_x's
        assert torch.equal(a[done], ra[done])
        assert torch.equal(_bits(lp)[done], _bits(rlp)[done])
        assert torch.equal(_bits(v)[done], _bits(rv)[done])
    assert bool(done.all())
    assert torch.equal(a, ra) and torch.equal(_bits(lp), _bits(rlp)) and torch.equal(_bits(v), _bits(rv))
    assert torch.equal(_bits(lg[:, 15].contiguous()), _bits(v))
    assert torch.equal(xb.view(torch.int16), xb0.view(torch.int16))


def _first_argmax(lg):
    acts, off = [], 0
    for n in HEADS:
        h = lg[:, off:off + n]
        best = torch.zeros((lg.shape[0],), dtype=torch.long, device=lg.device)
        bv = h[:, 0].clone()
        for k in range(1, n):  # strict > from index 0: the lowest index wins a tie
            up = h[:, k] > bv
            best = torch.where(up, torch.full_like(best, k), best)
            bv = torch.where(up, h[:, k], bv)
        acts.append(best)
        off += n
    return torch.stack(acts, dim=1).to(torch.int8)


@pytest.mark.parametrize('mask', [0b0011, 0b1111])
def test_greedy_is_the_argmax_of_its_own_logits(mask):
    D, A, N = 160, 4, 256
    p, fp = _fused(D, seed=2)
    M = N * A
    xb = _rows(fp, M, seed=3)
    sel = _selected(M, A, mask)
    a, lp, v, lg = _outputs(M, logits=True)
    fp.act_sel(xb, A, mask, 1, 2, a, lp, v, greedy=True, logits=lg)
    # logits_out against the torch fp32 forward on bf16-rounded weights and
    # inputs: |d| <= 0.03 + 0.03 |ref| (tests/test_gpu_policy.py's tolerance)
    ref = copy.deepcopy(p)
    with torch.no_grad():
        for prm in ref.parameters():
            prm.copy_(prm.bfloat16().float())
        raw = ref.forward_raw(xb[:, :D].float())
    torch.testing.assert_close(lg[sel], raw[sel], atol=0.03, rtol=0.03)
    assert torch.equal(a[sel], _first_argmax(lg[sel]))
    assert bool((a[~sel] == ACT_SENTINEL).all()) and bool((_bits(lp)[~sel] == NAN_BITS).all())
    # no RNG: another seed / step gives the same bits
    a2, lp2, v2, lg2 = _outputs(M, logits=True)
    fp.act_sel(xb, A, mask, 77, 9000, a2, lp2, v2, greedy=True, logits=lg2)
    assert torch.equal(a, a2) and torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(v), _bits(v2))
    assert torch.equal(_bits(lg), _bits(lg2))


def test_greedy_ties_take_the_lowest_index():
    D, A, N = 160, 4, 37
    p, fp = _fused(D, seed=4)
    with torch.no_grad():
        for prm in p.parameters():
            prm.zero_()
    fp.pack()
    M = N * A
    xb = _rows(fp, M, seed=5)
    a, lp, v, _ = _outputs(M)
    fp.act_sel(xb, A, 0b1111, 0, 0, a, lp, v, greedy=True)
    assert bool((a == 0).all())


def test_greedy_logp_has_the_samplers_bits():
    """Head bias +10 on option 1 of every head: the torch reference alone has a
    smallest top-two logit gap of 8.73 in every head (far above the logit
    tolerance), so greedy picks option 1 everywhere, and a sampled row equals
    the greedy row in >= 99.9 % of rows.  On the rows where the sampler drew
    the greedy choice, the two log-probs are the same bits."""
    D, M = 160, 1024
    torch.manual_seed(161)
    p = PolicyMLP(D).to(DEV)
    with torch.no_grad():
        p.head.bias.zero_()
        off = 0
        for n in HEADS:
            p.head.bias[off + 1] = 10.0
            off += n
    fp = FusedPolicy(p, D, torch.device(DEV))
    fp.pack()
    xb = _rows(fp, M, seed=5)
    ga, glp, gv, _ = _outputs(M)
    fp.act_sel(xb, 1, 0b1, 0, 0, ga, glp, gv, greedy=True)
    assert bool((ga == 1).all())
    sa, slp, sv, _ = _outputs(M)
    fp.act_sel(xb, 1, 0b1, 7, 3, sa, slp, sv)
    same = (sa == ga).all(1)
    assert float(same.float().mean()) >= 0.95
    assert torch.equal(_bits(slp)[same], _bits(glp)[same])
    assert torch.equal(_bits(sv), _bits(gv))


@pytest.mark.parametrize('A,mask', [(4, 0), (4, 0b10000), (0, 0b1)])
def test_invalid_arguments_raise_and_write_nothing(A, mask):
    D = 160
    _, fp = _fused(D, seed=6)
    M = 16
    xb = _rows(fp, M, seed=7)
    a, lp, v, lg = _outputs(M, logits=True)
    with pytest.raises(MasError):
        fp.act_sel(xb, A, mask, 0, 0, a, lp, v, logits=lg)
    torch.cuda.synchronize()
    assert bool((a == ACT_SENTINEL).all())
    for t in (lp, v, lg):
        assert bool((_bits(t) == NAN_BITS).all())
