"""PPOConfig.mask_dead on the fused path: 2v2 x 256 envs, horizon 16, two
minibatches.  The env is rolled out without updates until some but not all
rows of a rollout are active (dead agents appear once the zone closes: about
160 steps); on that rollout the fused gradient with row weights is compared
with autograd on policy_loss_reference(row_w=...) at the bars of
test_gpu_policy.py, the inactive rows' policy inputs are scrambled without
moving a bit of the gradient, and one update runs.  A self-play trainer with
the flag gathers `active` with the learner's other rows."""
import copy
import functools
import json
import os

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import (PolicyMLP, PPOConfig, PPOTrainer, chunk_row_weights, evaluate_actions,  # noqa: E402
                            policy_loss_reference)
from masurvival.vec_env import VecMaSurvival  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'configs', '2v2.json')) as _f:
    CFG_2V2 = json.load(_f)
N, T, MB = 256, 16, 2
MAX_ROLLOUTS = 20


def _rollout(tr):
    for t in range(tr.cfg.horizon):
        tr.rollout_step(t)
    tr.finish_rollout()


def _next_rollout(tr):
    """What update() does to the buffer between rollouts, without the update."""
    assert tr.x_obs
    tr.buf.xb[0].copy_(tr.buf.xb[tr.cfg.horizon])


def _bf16_ref(p):
    r = copy.deepcopy(p)
    with torch.no_grad():
        for prm in r.parameters():
            prm.copy_(prm.bfloat16().float())
            prm.grad = None
    return r


def _cos(a, b):
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _trainer():
    """The trainer after the first rollout with dead and alive rows (shared: the tests read it or restore it)."""
    env = VecMaSurvival(CFG_2V2, n_envs=N, seeds=range(N), auto_reset=True)
    tr = PPOTrainer(env, PPOConfig(horizon=T, minibatches=MB, mask_dead=True), seed=0)
    assert tr.fused is not None and tr.buf.active is not None
    for k in range(MAX_ROLLOUTS):
        _rollout(tr)
        share = float(tr.buf.active.mean())
        if share < 1.0:
            break
        _next_rollout(tr)
    torch.cuda.synchronize()
    print(f'rollout {k}: active share {share:.4f}, per minibatch {tr.buf.active_share.tolist()}')
    return tr, k


def _minibatch(tr, k):
    b = tr.buf
    tc = T // MB
    sl = slice(k * tc, (k + 1) * tc)
    M = tc * b.N * b.A
    return (b.xb[sl].reshape(M, tr.fused.Dx), b.actions[sl].reshape(M, 6), b.logp[sl].reshape(M),
            b.adv[sl].reshape(M), b.ret[sl].reshape(M)), b.row_w[sl].reshape(M), b.active[sl].reshape(M)


def _fused_grads(tr, batch, w):
    for q in tr.policy.parameters():
        if tr.fused_opt is None:
            q.grad = None
    st = tr.fused.grads(*batch, tr.cfg, row_w=w)
    torch.cuda.synchronize()
    return [float(s) for s in st], [q.grad.detach().clone() for q in tr.policy.parameters()]


def test_rollout_reaches_a_mixed_active_share():
    tr, k = _trainer()
    b = tr.buf
    share = float(b.active.mean())
    assert 0.0 < share < 1.0, (k, share)
    assert set(b.active.unique().tolist()) == {0.0, 1.0}
    # the weights: active * rows / sum(active) per time chunk, the shares their means
    w, s = chunk_row_weights(b.active, MB)
    assert torch.equal(w, b.row_w) and torch.equal(s, b.active_share)
    rows = b.active[0].numel() * (T // MB)
    for c in range(MB):
        a = b.active[c * (T // MB):(c + 1) * (T // MB)]
        assert float(b.row_w[c * (T // MB):(c + 1) * (T // MB)].sum()) == pytest.approx(rows, rel=1e-5)
        assert float(s[c]) == pytest.approx(float(a.mean()))
    # the advantages are normalised over the active rows
    a = b.adv[b.active.bool()].double()
    assert abs(float(a.mean())) < 1e-4 and abs(float(a.std(unbiased=False)) - 1.0) < 1e-3


def test_fused_weighted_gradient_matches_autograd_reference():
    tr, _ = _trainer()
    b, c = tr.buf, tr.cfg
    # the minibatch with the fewest active rows
    k = int(torch.argmin(b.active_share))
    batch, w, act = _minibatch(tr, k)
    assert 0 < int(act.sum()) < act.numel()
    xb, acts, old_lp, adv, ret = batch
    (loss, pg, vl, ent, cf), grads = _fused_grads(tr, batch, w)
    ref = _bf16_ref(tr.policy)
    x = xb[:, :b.D].float()
    rl, rpg, rvl, rent = policy_loss_reference(ref, x, acts, old_lp, adv, ret, c, row_w=w)
    rl.backward()
    for a, r in ((loss, rl), (pg, rpg), (vl, rvl), (ent, rent)):
        r = float(r.detach())
        assert abs(a - r) <= 0.02 + 0.02 * abs(r), (a, r)
    assert 0.0 <= cf <= 1.0
    for (name, _), ga, r in zip(tr.policy.named_parameters(), grads, ref.parameters()):
        gb = r.grad
        cos, rel = _cos(ga.float(), gb), float((ga.norm() - gb.norm()).abs() / gb.norm())
        print(f'{name}: cosine {cos:.6f} norm error {rel:.4%}')
        assert cos >= 0.999, (name, cos)
        assert rel <= 0.03, (name, rel)
    # the rollout's values and log-probs of these rows (the act kernel's): |d| <= 0.03 + 0.03 |ref|
    with torch.no_grad():
        raw = ref.forward_raw(x)
    tc = T // MB
    torch.testing.assert_close(b.values[k * tc:(k + 1) * tc].reshape(-1), raw[:, 15], atol=0.03, rtol=0.03)
    torch.testing.assert_close(old_lp, evaluate_actions(raw[:, :15], acts)[0], atol=0.03, rtol=0.03)


def test_scrambled_inactive_rows_leave_the_gradient_bit_identical():
    tr, _ = _trainer()
    k = int(torch.argmin(tr.buf.active_share))
    batch, w, act = _minibatch(tr, k)
    xb, acts, old_lp, adv, ret = batch
    st0, g0 = _fused_grads(tr, batch, w)
    g = torch.Generator(device='cuda').manual_seed(5)
    M = act.numel()
    off = act == 0
    hi = torch.tensor([3, 3, 3, 2, 2, 2], device='cuda')
    rnd = (torch.rand((M, 6), device='cuda', generator=g) * hi).long().clamp_(max=hi - 1).to(torch.int8)
    acts2 = torch.where(off[:, None], rnd, acts).contiguous()
    lp2 = torch.where(off, torch.full_like(old_lp, -200.0) * torch.rand(M, device='cuda', generator=g), old_lp)
    adv2 = torch.where(off, 1e30 * torch.randn(M, device='cuda', generator=g), adv)
    assert not torch.equal(acts2, acts)
    st1, g1 = _fused_grads(tr, (xb, acts2, lp2.contiguous(), adv2.contiguous(), ret), w)
    for a, b_ in zip(g0, g1):
        assert torch.equal(a, b_)
    assert st0 == st1


def test_iteration_with_mask_dead_runs():
    tr, _ = _trainer()
    before = [p.detach().clone() for p in tr.policy.parameters()]
    tr.update()
    torch.cuda.synchronize()
    assert 0.0 < float(tr.last_stats['active']) < 1.0
    for key in ('loss', 'pg', 'v', 'entropy', 'clipfrac'):
        assert bool(torch.isfinite(tr.last_stats[key])), key
    assert all(bool(torch.isfinite(p).all()) for p in tr.policy.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.policy.parameters()))
    tr.iteration()  # and a whole one from there
    torch.cuda.synchronize()
    assert 0.0 < float(tr.last_stats['active']) <= 1.0
    assert all(bool(torch.isfinite(p).all()) for p in tr.policy.parameters())
    _trainer.cache_clear()  # the shared rollout is gone
    tr.env.close()


def test_selfplay_gathers_active_with_the_learner_rows():
    n, t_, la = 64, 8, [0, 1]
    env = VecMaSurvival(CFG_2V2, n_envs=n, seeds=range(n), auto_reset=True)
    torch.manual_seed(77)
    sp = PPOTrainer(env, PPOConfig(horizon=t_, minibatches=MB, mask_dead=True), seed=0,
                    opponent=PolicyMLP(env.obs_dim, 256), learner_agents=la)
    lb = sp.buf.learner
    assert lb.active is not None and lb.active.shape == (t_, n, len(la))
    for k in range(2 * MAX_ROLLOUTS):
        _rollout(sp)
        if float(lb.active.mean()) < 1.0:
            break
        _next_rollout(sp)
    torch.cuda.synchronize()
    assert 0.0 < float(lb.active.mean()) < 1.0, k
    assert torch.equal(lb.active, sp.buf.active[:, :, la])
    assert torch.equal(lb.row_w, chunk_row_weights(lb.active, MB)[0])
    sp.update()
    sp.iteration()
    torch.cuda.synchronize()
    assert 0.0 < float(sp.last_stats['active']) <= 1.0
    assert all(bool(torch.isfinite(p).all()) for p in sp.policy.parameters())
    env.close()
