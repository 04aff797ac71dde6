"""Scripted bots in masurvival.match and in the self-play trainer, on the CPU:
a scripted env double whose rows look like the 2v2 config's observations
(tests/bot_rows.py) and do not depend on the actions, so two matches over it
see the same rows.  Bot sides must get exactly bot_actions_reference's
actions, the policy sides what they get without a bot, and the trainer's
checkpoint must name its bot."""
import pytest

torch = pytest.importorskip('torch')

import bot_rows  # noqa: E402
from masurvival.bots import BOT_KINDS, Bot, bot_actions_reference, parse_bot  # noqa: E402
from masurvival.config import C3_CONFIG, ResolvedConfig  # noqa: E402
from masurvival.match import Actor, Match  # noqa: E402
from masurvival.ppo import PolicyMLP, PPOConfig, PPOTrainer, gae_reference_into  # noqa: E402

N, A, STEPS = 6, 4, 5
RC = ResolvedConfig(C3_CONFIG)
D = bot_rows.layout_of(RC.to_struct())[0]


class RowsEnv:
    """Step k's observation is a fixed batch of synthetic rows; env e is done
    every e + 2 steps.  VecMaSurvival's reset / step (with out=) / state surface."""

    def __init__(self, n_envs=N, with_rc=True):
        self.n_envs, self.n_agents, self.obs_dim = n_envs, A, D
        self.device, self.auto_reset = torch.device('cpu'), True
        if with_rc:
            self.rc = RC
        cs = RC.to_struct()
        self.batches = [torch.from_numpy(bot_rows.random_rows(cs, n_envs, 100 + k)[:, :D].copy()).reshape(n_envs, A, D)
                        for k in range(16)]
        self.actions, self.k = [], 0

    def reset(self):
        self.k = 0
        return self.batches[0].clone()

    def step(self, actions, out=None):
        assert actions.shape == (self.n_envs, A, 6) and actions.dtype == torch.int8
        self.actions.append(actions.clone())
        self.k += 1
        obs = self.batches[self.k % len(self.batches)]
        rew = actions[..., 0].float() - 1.0 + actions[..., 3].float()
        done = ((self.k % (torch.arange(self.n_envs) + 2)) == 0).to(torch.uint8)
        if out is not None:
            out[0].copy_(obs), out[1].copy_(rew), out[2].copy_(done)
            return out[0], out[1], out[2], {}
        return obs.clone(), rew, done, {}

    def get_state(self):
        return torch.tensor([self.k], dtype=torch.int64).view(torch.uint8)

    def set_state(self, buf):
        self.k = int(buf.clone().view(torch.int64)[0])


def _policy(seed):
    torch.manual_seed(seed)
    return PolicyMLP(D)


def _history(policies, **kw):
    env = RowsEnv()
    m = Match(env, policies, **kw)
    m.run(steps=STEPS)
    return env, torch.stack(env.actions)  # [STEPS, N, A, 6]


@pytest.mark.parametrize('name', list(BOT_KINDS))
def test_bot_side_gets_exactly_the_reference_actions(name):
    env, hist = _history([_policy(0), 'bot:' + name])
    for t in range(STEPS):
        want = bot_actions_reference(name, env.batches[t], RC)
        assert torch.equal(hist[t][:, 2:], want[:, 2:]), t
    if name != 'idle':
        assert len(torch.unique(hist[:, :, 2:, 2])) == 3  # the rows make the bot turn both ways and hold


def test_policy_side_is_what_it_is_without_a_bot():
    # greedy: every step; the rows do not depend on the actions
    _, plain = _history([_policy(0), _policy(1)], greedy=True)
    _, mixed = _history([_policy(0), Bot('hunter')], greedy=True)
    assert torch.equal(plain[:, :, :2], mixed[:, :, :2])
    assert not torch.equal(plain[:, :, 2:], mixed[:, :, 2:])
    _, mixed = _history(['bot:forager', _policy(1)], greedy=True)
    assert torch.equal(plain[:, :, 2:], mixed[:, :, 2:])
    # sampled: side 0 draws first from the match's generator, so its first step is the same draw
    _, plain = _history([_policy(0), _policy(1)], seed=5)
    _, mixed = _history([_policy(0), 'bot:hunter'], seed=5)
    assert torch.equal(plain[0][:, :2], mixed[0][:, :2])


def test_swap_sides_inverts_the_masks():
    env, hist = _history([_policy(0), 'bot:hunter'], swap_sides=True, greedy=True)
    _, plain = _history([_policy(0), _policy(1)], swap_sides=True, greedy=True)
    h = N // 2
    for t in range(STEPS):
        want = bot_actions_reference('hunter', env.batches[t], RC)
        assert torch.equal(hist[t][:h, 2:], want[:h, 2:]) and torch.equal(hist[t][h:, :2], want[h:, :2]), t
    assert torch.equal(hist[:, :h, :2], plain[:, :h, :2]) and torch.equal(hist[:, h:, 2:], plain[:, h:, 2:])


def test_two_bots_and_one_bot():
    env, hist = _history(['bot:hunter', Bot('forager')])
    for t in range(STEPS):
        assert torch.equal(hist[t][:, :2], bot_actions_reference('hunter', env.batches[t], RC)[:, :2])
        assert torch.equal(hist[t][:, 2:], bot_actions_reference('forager', env.batches[t], RC)[:, 2:])
    env, hist = _history(['bot:hunter'])
    assert torch.equal(hist[0], bot_actions_reference('hunter', env.batches[0], RC))
    m = Match(RowsEnv(), ['bot:hunter', 'bot:idle'])
    res = m.run(steps=12)
    assert res['episodes'] > 0 and res['steps'] == 12 and sum(res['wins']) + res['draws'] == res['episodes']


def test_refusals():
    for bad in ('bot:nope', 'bot:', 'bot:HUNTER'):
        with pytest.raises(ValueError, match='unknown bot'):
            parse_bot(bad)
        with pytest.raises(ValueError, match='unknown bot'):
            Match(RowsEnv(), [_policy(0), bad])
    with pytest.raises(ValueError, match='config'):
        Match(RowsEnv(with_rc=False), [_policy(0), 'bot:hunter'])
    with pytest.raises(ValueError, match='config'):
        Actor(['bot:hunter'], N, A, D, 'cpu')
    with pytest.raises(ValueError, match='n_agents'):
        Actor(['bot:hunter'], N, 2, D, 'cpu', config=RC)
    # without a bot nothing asks for a config
    Match(RowsEnv(with_rc=False), [_policy(0), _policy(1)]).run(steps=2)


# -- the self-play trainer ---------------------------------------------------

T = 4


def _trainer(opponent='bot:hunter', env=None, **kw):
    cfg = PPOConfig(horizon=T, hidden=32, minibatches=2, autocast_bf16=False, **kw)
    tr = PPOTrainer(env if env is not None else RowsEnv(8), cfg, seed=3, opponent=opponent, learner_agents=[0, 1])
    tr.gae_impl = gae_reference_into
    return tr


def test_trainer_bot_fills_the_opponent_rows():
    tr = _trainer()
    assert tr.opponent is None and tr.opponent_bot == Bot('hunter') and tr.learner_agents == [0, 1]
    b = tr.buf
    for t in range(T):
        tr.rollout_step(t)
    for t in range(T):  # (before the update: it moves the last observation into obs[0])
        want = bot_actions_reference('hunter', b.obs[t], RC)
        assert torch.equal(b.actions[t][:, 2:], want[:, 2:]), t
    # the learner's rows are the learner's draws: the same as against a policy opponent, which draws after it
    torch.manual_seed(11)
    other = _trainer(opponent=PolicyMLP(D, 32))
    other.rollout_step(0)
    tr2 = _trainer()
    tr2.rollout_step(0)
    assert torch.equal(other.buf.actions[0][:, :2], tr2.buf.actions[0][:, :2])
    assert torch.equal(other.buf.logp[0], tr2.buf.logp[0])


def test_trainer_checkpoint_round_trip_names_the_bot(tmp_path):
    a = _trainer()
    a.iteration()
    sd = a.state_dict()
    assert sd['opponent_bot'] == 'hunter' and 'opponent' not in sd and sd['learner_agents'] == [0, 1]
    path = tmp_path / 'bot.pt'
    a.save(str(path))
    b = _trainer()
    b.load(str(path))
    a.iteration()
    b.iteration()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(a.buf.actions, b.buf.actions)


def test_trainer_refusals():
    with pytest.raises(ValueError, match='unknown bot'):
        _trainer(opponent='bot:sniper')
    with pytest.raises(ValueError, match='opponent_sync_every'):
        _trainer(opponent_sync_every=1)
    with pytest.raises(ValueError, match='config'):
        _trainer(env=RowsEnv(8, with_rc=False))
    tr = _trainer()
    with pytest.raises(ValueError, match='bot'):
        tr.sync_opponent()
    with pytest.raises(ValueError, match='proper subset'):
        PPOTrainer(RowsEnv(8), PPOConfig(horizon=T, hidden=32), opponent='bot:hunter', learner_agents=range(A))
    sd = tr.state_dict()
    with pytest.raises(ValueError, match='opponent bot'):
        _trainer(opponent='bot:forager').load_state_dict(sd)
    torch.manual_seed(11)
    pol = _trainer(opponent=PolicyMLP(D, 32))
    with pytest.raises(ValueError, match='opponent bot'):
        pol.load_state_dict(sd)           # a bot's checkpoint into a policy opponent's trainer
    with pytest.raises(ValueError, match='opponent'):
        tr.load_state_dict(pol.state_dict())   # and the other way round
    plain = PPOTrainer(RowsEnv(8), PPOConfig(horizon=T, hidden=32, autocast_bf16=False), seed=3)
    with pytest.raises(ValueError):
        plain.load_state_dict(sd)
