"""Self-play on the torch path of PPOTrainer (opponent= / learner_agents=):
a frozen opponent drives the agents the learner does not own, and GAE, the
advantage statistics and the update see the learner's rows alone.  CPU only,
on a scripted env double (the StandInEnv of tests/test_ppo.py, restated)."""
import copy

import pytest

torch = pytest.importorskip('torch')

from masurvival.ppo import PolicyMLP, PPOConfig, PPOTrainer, gae_reference, gae_reference_into  # noqa: E402

T, N, A, D = 6, 8, 4, 12


class StandInEnv:
    """Deterministic CPU env with VecMaSurvival's step / reset / get_state surface."""

    def __init__(self, n_envs=N, n_agents=A, obs_dim=D, seed=0):
        self.n_envs, self.n_agents, self.obs_dim = n_envs, n_agents, obs_dim
        self.device = torch.device('cpu')
        self.g = torch.Generator().manual_seed(seed)
        self.t = 0

    def reset(self):
        return torch.randn((self.n_envs, self.n_agents, self.obs_dim), generator=self.g)

    def step(self, actions, out=None):
        self.t += 1
        o, r, d = out
        o.copy_(torch.randn(o.shape, generator=self.g))
        r.copy_((actions[..., 0].float() - 1.0) * 0.5 + (actions[..., 3].float()))
        d.copy_(((torch.arange(self.n_envs) + self.t) % 5 == 0).to(torch.uint8))
        return o, r, d, {}

    def get_state(self):
        return torch.cat([self.g.get_state(), torch.tensor([self.t], dtype=torch.int64).view(torch.uint8)])

    def set_state(self, buf):
        self.g.set_state(buf[:-8].clone())
        self.t = int(buf[-8:].clone().view(torch.int64)[0])


def _cfg(**kw):
    return PPOConfig(horizon=T, hidden=32, minibatches=2, autocast_bf16=False, **kw)


def _trainer(env=None, cfg=None, **kw):
    tr = PPOTrainer(env if env is not None else StandInEnv(), cfg if cfg is not None else _cfg(), seed=3, **kw)
    tr.gae_impl = gae_reference_into
    return tr


def _opponent(seed=11):
    torch.manual_seed(seed)
    return PolicyMLP(D, 32)


def _same(ps, qs):
    ps, qs = list(ps), list(qs)
    return len(ps) == len(qs) and all(torch.equal(p, q) for p, q in zip(ps, qs))


def test_full_learner_set_without_opponent_is_the_plain_trainer():
    plain, sel = _trainer(), _trainer(learner_agents=range(A))
    assert plain.buf.learner is None and sel.buf.learner is not None
    for _ in range(2):
        plain.iteration()
        sel.iteration()
    assert _same(plain.policy.parameters(), sel.policy.parameters())
    assert torch.equal(plain.gen.get_state(), sel.gen.get_state())  # the generator was consumed alike
    s1, s2 = plain.opt.state_dict()['state'], sel.opt.state_dict()['state']
    for k in s1:
        assert torch.equal(s1[k]['exp_avg'], s2[k]['exp_avg']) and torch.equal(s1[k]['exp_avg_sq'], s2[k]['exp_avg_sq'])


def test_plain_trainer_has_no_selfplay_state():
    tr = _trainer()
    assert tr.opponent is None and tr.learner_agents is None and tr.buf.learner is None
    assert 'opponent' not in tr.state_dict() and 'learner_agents' not in tr.state_dict()


def test_default_learner_agents_are_side_0():
    assert _trainer(opponent=_opponent()).learner_agents == [0, 1]


@pytest.mark.parametrize('learner', [None, [1, 3], [2]])
def test_opponent_is_frozen_and_learner_rows_are_compacted(learner):
    opp = _opponent()
    tr = _trainer(opponent=opp, learner_agents=learner)
    assert tr.opponent is not opp and _same(tr.opponent.parameters(), opp.parameters())  # a deep copy
    assert not tr.opponent.training and not any(p.requires_grad for p in tr.opponent.parameters())
    opt_ids = {id(p) for g in tr.opt.param_groups for p in g['params']}
    assert not opt_ids & {id(p) for p in tr.opponent.parameters()}
    before = [p.detach().clone() for p in tr.policy.parameters()]
    for t in range(T):
        tr.rollout_step(t)
    tr.finish_rollout()
    b, lb = tr.buf, tr.buf.learner
    la = tr.learner_agents
    m = len(la)
    assert lb.A == m and float(lb.adv_stats[2]) == T * N * m
    assert torch.equal(lb.obs[:T], b.obs[:T][:, :, la])
    for name in ('actions', 'logp', 'rewards', 'values'):
        assert torch.equal(getattr(lb, name), getattr(b, name)[:, :, la]), name
    # GAE on the compact columns with n_agents = m (before the normalisation: recomputed here)
    adv, ret = gae_reference(lb.rewards, lb.values, b.dones, tr.cfg.gamma, tr.cfg.lam, m)
    assert torch.equal(lb.ret, ret)
    mean, std = adv.double().mean(), adv.double().var(unbiased=False).sqrt()
    torch.testing.assert_close(lb.adv, ((adv - mean.float()) / (std.float() + 1e-8)), atol=1e-5, rtol=1e-5)
    tr.update()
    assert _same(tr.opponent.parameters(), opp.parameters())
    assert not _same(tr.policy.parameters(), before)
    assert torch.equal(b.obs[0], b.obs[T])  # the carry stays on the full buffer


def test_opponent_actions_come_from_the_opponent():
    """The actions of the opponent's agents are its own draw from the shared
    generator, the learner's are the learner's."""
    opp = _opponent()
    tr = _trainer(opponent=opp, learner_agents=[0, 2])
    twin = _trainer(opponent=opp, learner_agents=[0, 2])
    tr.rollout_step(0)
    from masurvival.ppo import sample_actions
    with torch.no_grad():
        la, _ = sample_actions(twin.policy(twin.buf.obs[0])[0], twin.gen)
        oa, _ = sample_actions(opp(twin.buf.obs[0])[0], twin.gen)
    assert torch.equal(tr.buf.actions[0][:, [0, 2]], la[:, [0, 2]])
    assert torch.equal(tr.buf.actions[0][:, [1, 3]], oa[:, [1, 3]])


def test_sync_opponent_and_sync_every():
    tr = _trainer(opponent=_opponent())
    tr.iteration()
    assert not _same(tr.opponent.parameters(), tr.policy.parameters())
    tr.sync_opponent()
    assert _same(tr.opponent.parameters(), tr.policy.parameters())
    assert not any(p.requires_grad for p in tr.opponent.parameters())
    tr2 = _trainer(cfg=_cfg(opponent_sync_every=1), opponent=_opponent())
    tr2.iteration()
    assert _same(tr2.opponent.parameters(), tr2.policy.parameters()) and tr2.iterations == 1
    tr3 = _trainer(cfg=_cfg(opponent_sync_every=2), opponent=_opponent())
    tr3.iteration()
    assert not _same(tr3.opponent.parameters(), tr3.policy.parameters())
    tr3.iteration()
    assert _same(tr3.opponent.parameters(), tr3.policy.parameters())
    with pytest.raises(ValueError):
        _trainer().sync_opponent()


def test_checkpoint_resume_continues_the_same_trajectory(tmp_path):
    cfg = _cfg(opponent_sync_every=3)
    tr = _trainer(cfg=cfg, opponent=_opponent(), learner_agents=[1, 2])
    tr.iteration()
    path = str(tmp_path / 'ckpt.pt')
    tr.save(path)
    sd = torch.load(path, weights_only=True)  # tensors and plain numbers only
    assert sd['learner_agents'] == [1, 2] and sd['iterations'] == 1 and 'opponent' in sd
    tr2 = _trainer(env=StandInEnv(seed=99), cfg=cfg, opponent=_opponent(seed=12), learner_agents=[1, 2])
    tr2.load(path)
    assert _same(tr2.opponent.parameters(), tr.opponent.parameters()) and tr2.iterations == 1
    for _ in range(2):  # the second one crosses the opponent sync
        tr.iteration()
        tr2.iteration()
    assert _same(tr.policy.parameters(), tr2.policy.parameters())
    assert _same(tr.opponent.parameters(), tr2.opponent.parameters())
    assert _same(tr.opponent.parameters(), tr.policy.parameters())
    assert torch.equal(tr.buf.obs[0], tr2.buf.obs[0]) and tr.steps_taken == tr2.steps_taken
    # 'policy' stays the learner: read as any checkpoint's
    from masurvival.match import load_policy
    assert _same(load_policy(path).parameters(), torch.load(path, weights_only=True)['policy'].values())


def test_checkpoint_with_other_learner_agents_is_refused(tmp_path):
    tr = _trainer(opponent=_opponent(), learner_agents=[0, 1])
    path = str(tmp_path / 'ckpt.pt')
    tr.save(path)
    with pytest.raises(ValueError, match='learner_agents'):
        _trainer(opponent=_opponent(), learner_agents=[0, 2]).load(path)
    with pytest.raises(ValueError, match='learner_agents'):
        _trainer().load(path)
    plain = str(tmp_path / 'plain.pt')
    _trainer().save(plain)
    with pytest.raises(ValueError, match='learner_agents'):
        _trainer(opponent=_opponent()).load(plain)


def test_opponent_from_a_checkpoint_path_or_dict(tmp_path):
    opp = _opponent()
    path = str(tmp_path / 'opp.pt')
    torch.save({'policy': opp.state_dict()}, path)
    for src in (path, {'policy': copy.deepcopy(opp.state_dict())}):
        tr = _trainer(opponent=src)
        assert _same(tr.opponent.parameters(), opp.parameters())


@pytest.mark.parametrize('kw', [
    dict(learner_agents=[0, 1]),                                  # a proper subset without an opponent
    dict(learner_agents=[]),                                      # empty
    dict(learner_agents=[0, 0, 1, 2]),                            # repeated
    dict(learner_agents=[0, 4]),                                  # out of range
    dict(learner_agents=[-1]),
    dict(opponent='yes', learner_agents=[0, 1, 2, 3]),            # not a proper subset
    dict(opponent='yes', learner_agents=[]),
    dict(opponent='yes', learner_agents=[1, 1]),
    dict(opponent='yes', learner_agents=[7]),
])
def test_bad_learner_agents_raise(kw):
    if kw.get('opponent') == 'yes':
        kw = dict(kw, opponent=_opponent())
    with pytest.raises(ValueError):
        _trainer(**kw)


def test_opponent_obs_dim_mismatch_raises():
    torch.manual_seed(0)
    with pytest.raises(ValueError, match='obs_dim'):
        _trainer(opponent=PolicyMLP(D + 1, 32))
    with pytest.raises(ValueError, match='obs_dim'):
        _trainer(opponent={'policy': PolicyMLP(D + 1, 32).state_dict()})


def test_one_agent_env_has_no_default_learner():
    with pytest.raises(ValueError):
        _trainer(env=StandInEnv(n_agents=1), opponent=_opponent())
