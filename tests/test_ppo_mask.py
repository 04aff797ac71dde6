"""PPOConfig.mask_dead on the CPU / torch path: the weighted loss against a
hand-written masked one, the per-minibatch weights (a minibatch without an
active row gives zeros, never NaN), the constructor's refusal of an env
without alive(), and one iteration() on a stand-in env with alive()."""
import pytest
import torch

from masurvival.ppo import (PolicyMLP, PPOConfig, PPOTrainer, chunk_row_weights, evaluate_actions,
                            gae_reference_into, masked_mean, policy_loss_reference, sample_actions)
from test_ppo import StandInEnv


class AliveStandInEnv(StandInEnv):
    """StandInEnv whose agents die: agent a of env e is dead from step 2 + (e + a) % 4
    of each 5-step episode of env e on (test double)."""

    def alive(self, out=None):
        e = torch.arange(self.n_envs)[:, None]
        a = torch.arange(self.n_agents)[None, :]
        age = (e + self.t) % 5  # steps since env e's last done flag
        al = (age < 2 + (e + a) % 4).float()
        if out is None:
            return al
        out.copy_(al)
        return out


def _batch(M=64, D=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    p = PolicyMLP(D, 32)
    x = torch.randn((M, D), generator=g)
    acts, lp = sample_actions(p(x)[0].detach(), g)
    old_lp = lp + 0.3 * torch.randn((M,), generator=g)
    adv = torch.randn((M,), generator=g)
    ret = torch.randn((M,), generator=g)
    return p, x, acts, old_lp, adv, ret, g


def test_weighted_reference_loss_is_the_hand_written_masked_loss():
    p, x, acts, old_lp, adv, ret, g = _batch()
    cfg = PPOConfig()
    M = x.shape[0]
    active = (torch.rand(M, generator=g) >= 1.0 / 3.0).float()
    assert 0 < int(active.sum()) < M
    w, share = chunk_row_weights(active, 1)
    loss, pg, vl, ent = policy_loss_reference(p, x, acts, old_lp, adv, ret, cfg, row_w=w)
    # by hand: policy terms averaged over the active rows, the value term over all rows
    on = active.bool()
    logits, v = p(x)
    lp, e = evaluate_actions(logits, acts)
    ratio = torch.exp(lp - old_lp)
    sur = torch.min(ratio * adv, ratio.clamp(1 - cfg.clip, 1 + cfg.clip) * adv)
    pg_h = -sur[on].mean()
    ent_h = e[on].mean()
    vl_h = ((v - ret) ** 2).mean()
    torch.testing.assert_close(pg, pg_h, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ent, ent_h, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(vl, vl_h, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(loss, pg_h + cfg.vf_coef * vl_h - cfg.ent_coef * ent_h, rtol=1e-5, atol=1e-6)
    assert float(share[0]) == pytest.approx(float(active.mean()))
    # the inactive rows' policy inputs do not reach the gradient
    loss.backward()
    g0 = [q.grad.clone() for q in p.parameters()]
    old2 = torch.where(on, old_lp, torch.full_like(old_lp, -200.0))  # the ratio overflows there
    adv2 = torch.where(on, adv, torch.full_like(adv, -1e30))
    for q in p.parameters():
        q.grad = None
    loss2 = policy_loss_reference(p, x, acts, old2, adv2, ret, cfg, row_w=w)[0]
    loss2.backward()
    assert torch.isfinite(loss2)
    for a, q in zip(g0, p.parameters()):
        assert torch.equal(a, q.grad)
    # without weights the reference is what it was
    l0 = policy_loss_reference(p, x, acts, old_lp, adv, ret, cfg)
    l1 = policy_loss_reference(p, x, acts, old_lp, adv, ret, cfg, row_w=torch.ones(M))
    for a, b in zip(l0, l1):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


def test_chunk_weights_normalise_per_chunk_and_survive_an_empty_chunk():
    active = torch.tensor([[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 1]], dtype=torch.float32)
    w, share = chunk_row_weights(active.reshape(2, 2, 4), 4)
    assert w.shape == (2, 2, 4)
    w = w.reshape(4, 4)
    assert torch.equal(w[0], torch.tensor([4 / 3, 0, 4 / 3, 4 / 3]))
    assert torch.equal(w[1], torch.zeros(4))  # no active row: zeros, not NaN
    assert torch.equal(w[2], torch.ones(4))
    assert torch.equal(w[3], torch.tensor([0.0, 0, 0, 4]))
    assert torch.equal(share, torch.tensor([0.75, 0.0, 1.0, 0.25]))
    assert bool(torch.isfinite(w).all())
    # every chunk with an active row sums to its row count: sum(w x) / rows is the mean over the active rows
    assert torch.equal(w.sum(1), torch.tensor([4.0, 0.0, 4.0, 4.0]))
    x = torch.tensor([1.0, float('inf'), 3.0, 5.0])
    assert float(masked_mean(x, w[0])) == pytest.approx(3.0)
    assert float(masked_mean(x, w[1])) == 0.0


def test_mask_dead_needs_an_env_with_alive():
    with pytest.raises(ValueError, match='alive'):
        PPOTrainer(StandInEnv(), PPOConfig(horizon=6, hidden=32, minibatches=2, autocast_bf16=False, mask_dead=True))
    assert PPOConfig().mask_dead is False
    tr = PPOTrainer(StandInEnv(), PPOConfig(horizon=6, hidden=32, minibatches=2, autocast_bf16=False))
    assert tr.buf.active is None


def test_trainer_iteration_with_mask_dead_cpu():
    env = AliveStandInEnv()
    tr = PPOTrainer(env, PPOConfig(horizon=6, hidden=32, minibatches=2, autocast_bf16=False, mask_dead=True), seed=3)
    tr.gae_impl = gae_reference_into
    before = [p.detach().clone() for p in tr.policy.parameters()]
    tr.iteration()
    b = tr.buf
    act = b.active
    assert act.shape == (6, env.n_envs, env.n_agents) and set(act.unique().tolist()) == {0.0, 1.0}
    # active[t] is alive() before step t (the env's t counts its steps)
    env2 = AliveStandInEnv()
    for t in range(6):
        assert torch.equal(act[t], env2.alive())
        env2.t += 1
    assert 0.0 < float(tr.last_stats['active']) < 1.0
    assert torch.isfinite(tr.last_stats['loss'])
    assert any(not torch.equal(a, c) for a, c in zip(before, tr.policy.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in tr.policy.parameters())
    # the advantages are normalised over the active rows
    a = b.adv[act.bool()].double()
    assert abs(float(a.mean())) < 1e-4 and abs(float(a.std(unbiased=False)) - 1) < 1e-3
    assert abs(float(b.adv.mean())) > 1e-4  # and not over all rows
