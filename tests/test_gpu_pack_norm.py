"""mas_policy_pack_norm: the observation normaliser folded into the packed
layer-1 weights, for D in {138, 160, 468} (9, 10 and 30 layer-1 k-steps; 138
leaves a partial k-step).

The host fold the images are held against, bit for bit:
  W1f = (W1 * s).bfloat16().float()        an fp32 product, rounded once
  b1' = float(b1 - sum_k W1f[:, k] * mu[k]) in fp64 over ascending k
and a plain mas_policy_pack of (W1f, b1', W2, b2, W3, b3).  Since the images
are equal, everything computed from them is: the act kernels' outputs and the
train kernel's stores; the layer-1 weight gradient is then unfolded on the
host (unfold_dw1), two elementwise fp32 ops."""
import copy
import ctypes

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import FusedPolicy, PolicyMLP, PPOConfig, evaluate_actions, unfold_dw1  # noqa: E402

DIMS = [138, 160, 468]
DEV = torch.device('cuda')


def _case(D):
    """(policy with a normaliser, the host-folded plain policy), on the GPU:
    |mean| up to 100, inv_std in [0.05, 10]."""
    torch.manual_seed(D)
    p = PolicyMLP(D, 256).to(DEV)
    g = torch.Generator().manual_seed(1000 + D)
    mean = ((torch.rand((D,), generator=g) * 2 - 1) * 100).to(DEV)
    s = (0.05 + torch.rand((D,), generator=g) * 9.95).to(DEV)
    mean[0], s[0], s[1] = 100.0, 10.0, 0.05
    folded = copy.deepcopy(p)
    with torch.no_grad():
        w1f = (p.body[0].weight * s).bfloat16().float()
        acc = torch.zeros((256,), dtype=torch.float64, device=DEV)
        for k in range(D):  # ascending k, every product exact
            acc += w1f[:, k].double() * mean[k].double()
        folded.body[0].weight.copy_(w1f)
        folded.body[0].bias.copy_((p.body[0].bias.double() - acc).float())
    p.set_obs_norm(mean, s)
    return p, folded


def _packed(policy, D):
    fp = FusedPolicy(policy, D, DEV)
    fp.packed.fill_(0xA5)
    fp.pack()
    return fp


def _raw_rows(fp, policy, M, seed):
    """bf16 rows [M, Dx] whose normalised values are O(1): mean + randn / s."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = fp.x_buffer(M)
    z = torch.randn((M, fp.D), device='cuda', generator=g)
    x[:, :fp.D] = (policy.obs_mean + z / policy.obs_inv_std).to(torch.bfloat16)
    return x


@pytest.mark.parametrize('D', DIMS)
def test_null_statistics_are_mas_policy_pack_byte_for_byte(D):
    _, folded = _case(D)
    fp = _packed(folded, D)
    other = torch.full_like(fp.packed, 0x5A)
    p = folded
    ts = [t.detach().float().contiguous() for t in (p.body[0].weight, p.body[0].bias, p.body[2].weight,
                                                   p.body[2].bias, p.head.weight, p.head.bias)]
    rc = fp.lib.mas_policy_pack_norm(D, *[ctypes.c_void_p(t.data_ptr()) for t in ts], None, None,
                                     ctypes.c_void_p(other.data_ptr()), fp._stream())
    assert rc == 0
    assert torch.equal(other, fp.packed)


@pytest.mark.parametrize('D', DIMS)
def test_fold_equals_the_pack_of_the_host_folded_parameters(D):
    normed, folded = _case(D)
    a, b = _packed(normed, D), _packed(folded, D)
    assert torch.equal(a.packed, b.packed)
    # and it is a fold: not the image of the unfolded weights
    plain = copy.deepcopy(normed)
    plain.set_obs_norm(None, None)
    assert not torch.equal(_packed(plain, D).packed, a.packed)


def _act_out(M):
    return (torch.empty((M, 6), dtype=torch.int8, device='cuda'), torch.empty((M,), device='cuda'),
            torch.empty((M,), device='cuda'))


@pytest.mark.parametrize('M', [32 * 3 + 5, 1013])
@pytest.mark.parametrize('D', DIMS)
def test_act_outputs_are_bit_identical_to_the_host_folded_policy(D, M):
    normed, folded = _case(D)
    a, b = _packed(normed, D), _packed(folded, D)
    x = _raw_rows(a, normed, M, seed=M)
    oa, ob = _act_out(M), _act_out(M)
    a.act_x(x, 11, 5, *oa)
    b.act_x(x, 11, 5, *ob)
    for u, v in zip(oa, ob):
        assert torch.equal(u, v)
    la, lb = torch.empty((M, 16), device='cuda'), torch.empty((M, 16), device='cuda')
    a.act_sel(x, 1, 1, 11, 5, *_act_out(M), logits=la)
    b.act_sel(x, 1, 1, 11, 5, *_act_out(M), logits=lb)
    assert torch.equal(la, lb) and bool(torch.isfinite(la).all())


@pytest.mark.parametrize('D', DIMS)
def test_act_against_the_fp32_forward_of_the_normalised_policy(D):
    """value and logp against the fp32 torch forward with the bf16-rounded
    folded weights on the same rows: atol = rtol = 0.03, the criterion of
    test_gpu_policy.test_policy_act_matches_reference."""
    M = 1013
    normed, folded = _case(D)
    a = _packed(normed, D)
    x = _raw_rows(a, normed, M, seed=3)
    acts, lp, v = _act_out(M)
    a.act_x(x, 11, 5, acts, lp, v)
    ref = copy.deepcopy(folded)
    with torch.no_grad():
        for prm in ref.parameters():
            prm.copy_(prm.bfloat16().float())
        ref.body[0].bias.copy_(folded.body[0].bias)  # the kernels keep biases in fp32
        ref.body[2].bias.copy_(folded.body[2].bias)
        ref.head.bias.copy_(folded.head.bias)
        raw = ref.forward_raw(x[:, :D].float())
    torch.testing.assert_close(v, raw[:, 15], atol=0.03, rtol=0.03)
    ref_lp, _ = evaluate_actions(raw[:, :15], acts)
    torch.testing.assert_close(lp, ref_lp, atol=0.03, rtol=0.03)


@pytest.mark.parametrize('D', DIMS)
def test_grads_are_the_plain_ones_with_dw1_unfolded(D):
    M = 2048
    normed, folded = _case(D)
    a, b = _packed(normed, D), _packed(folded, D)
    x = _raw_rows(a, normed, M, seed=9)
    acts, lp, v = _act_out(M)
    b.act_x(x, 11, 5, acts, lp, v)
    g = torch.Generator(device='cuda').manual_seed(D)
    adv = torch.randn((M,), device='cuda', generator=g)
    ret = v + 0.5 * torch.randn((M,), device='cuda', generator=g)
    cfg = PPOConfig()
    sa = a.grads(x, acts, lp, adv, ret, cfg)
    sb = b.grads(x, acts, lp, adv, ret, cfg)
    for u, w in zip(sa, sb):
        assert torch.equal(u, w)
    pa, pb = dict(normed.named_parameters()), dict(folded.named_parameters())
    for name in ('body.0.bias', 'body.2.weight', 'body.2.bias', 'head.weight', 'head.bias'):
        assert torch.equal(pa[name].grad, pb[name].grad), name
    want = unfold_dw1(pb['body.0.weight'].grad.double(), pb['body.0.bias'].grad.double(),
                      normed.obs_mean.double(), normed.obs_inv_std.double())
    got = pa['body.0.weight'].grad.double()
    assert bool(torch.isfinite(got).all())
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6 * float(want.abs().max()))
    assert not torch.equal(pa['body.0.weight'].grad, pb['body.0.weight'].grad)
