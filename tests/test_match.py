"""masurvival.match on the CPU: the score keeping against hand-computed values
on a scripted env double (fixed per-step rewards and episode lengths), the
argument errors, load_policy and the greedy mode's independence of the seed.

The double: 6 envs x 4 agents, env e pays agent a REWARDS[e][a] every step and
is done (and resets itself) every LENGTHS[e] steps.  Ten steps finish
5 + 3 + 2 + 5 + 2 + 0 = 17 episodes of 10 + 9 + 8 + 10 + 10 = 47 steps; env 5's
episode never finishes and must not be counted."""
import pytest

torch = pytest.importorskip('torch')

from masurvival.match import Match, load_policy  # noqa: E402
from masurvival.ppo import PolicyMLP  # noqa: E402

REWARDS = [[1, 0, 0, 0],
           [0, 0, 1, 1],
           [1, 1, 1, 1],
           [2, 0, 0, 1],
           [0, 1, 0, 0.5],
           [0, 0, 0, 3]]
LENGTHS = [2, 3, 4, 2, 5, 100]
D = 8


class ScriptedEnv:
    def __init__(self, n_envs=6, auto_reset=True, obs_dim=D):
        self.n_envs, self.n_agents, self.obs_dim = n_envs, 4, obs_dim
        self.device, self.auto_reset = torch.device('cpu'), auto_reset
        self.R = torch.tensor(REWARDS[:n_envs], dtype=torch.float32)
        self.L = torch.tensor(LENGTHS[:n_envs])
        g = torch.Generator().manual_seed(1)
        self.base = torch.randn((n_envs, 4, obs_dim), generator=g)
        self.actions = []

    def _obs(self, last=None):
        o = self.base * float(torch.cos(torch.tensor(0.3 * self.k)))
        return o if last is None else o + 0.25 * last.float().sum(-1, keepdim=True)

    def reset(self):
        self.t = torch.zeros((self.n_envs,), dtype=torch.long)
        self.k = 0
        return self._obs()

    def step(self, actions):
        assert actions.shape == (self.n_envs, 4, 6) and actions.dtype == torch.int8
        self.actions.append(actions.clone())
        self.t += 1
        self.k += 1
        done = self.t >= self.L
        self.t[done] = 0
        return self._obs(actions), self.R.clone(), done.to(torch.uint8), {}


def _policy(seed, obs_dim=D):
    torch.manual_seed(seed)
    return PolicyMLP(obs_dim)


def _check(res, wins, draws, ret):
    assert res['episodes'] == 17 and res['steps'] == 10
    assert res['wins'] == wins and res['draws'] == draws
    assert res['return'] == pytest.approx([ret[0] / 17, ret[1] / 17], rel=1e-12)
    assert res['mean_length'] == pytest.approx(47 / 17, rel=1e-12)
    assert set(res) == {'episodes', 'steps', 'wins', 'draws', 'return', 'mean_length'}
    assert all(type(w) is int for w in res['wins']) and all(type(r) is float for r in res['return'])


def test_default_assignment_is_the_team_split():
    # sides (a0 + a1, a2 + a3) per episode: e0 (2, 0) x5, e1 (0, 6) x3, e2 (8, 8) x2 draws,
    # e3 (4, 2) x5, e4 (5, 2.5) x2
    m = Match(ScriptedEnv(), [_policy(0), _policy(1)])
    _check(m.run(steps=10), [12, 3], 2, (10 + 0 + 16 + 20 + 10, 0 + 18 + 16 + 10 + 5))


def test_explicit_assignment():
    # sides (a0 + a2, a1 + a3): e0 (2, 0) x5, e1 (3, 3) x3 draws, e2 (8, 8) x2 draws,
    # e3 (4, 2) x5, e4 (0, 7.5) x2
    m = Match(ScriptedEnv(), [_policy(0), _policy(1)], assignment=[0, 1, 0, 1])
    _check(m.run(steps=10), [10, 2], 5, (10 + 9 + 16 + 20 + 0, 0 + 9 + 16 + 10 + 15))


def test_swap_sides_inverts_the_second_half_of_the_envs():
    # envs 3..5 play (a2 + a3, a0 + a1): e3 (2, 4) x5, e4 (2.5, 5) x2
    m = Match(ScriptedEnv(), [_policy(0), _policy(1)], swap_sides=True)
    _check(m.run(steps=10), [5, 10], 2, (10 + 0 + 16 + 10 + 5, 0 + 18 + 16 + 20 + 10))


def test_one_policy_defaults_to_one_side():
    m = Match(ScriptedEnv(), [_policy(0)])
    res = m.run(steps=10)
    # every agent on side 0: side 1's return is 0, side 0 wins every episode
    assert res['wins'] == [17, 0] and res['draws'] == 0 and res['return'][1] == 0.0
    assert res['return'][0] == pytest.approx((10 + 18 + 32 + 30 + 15) / 17)


def test_step_returns_rewards_and_dones_and_unfinished_episodes_are_not_counted():
    m = Match(ScriptedEnv(), [_policy(0), _policy(1)])
    r, d = m.step()
    assert tuple(r.shape) == (6, 4) and tuple(d.shape) == (6,) and not bool(d.any())
    assert m.result()['episodes'] == 0 and m.result()['return'] == [0.0, 0.0]
    r, d = m.step()
    assert d.tolist() == [1, 0, 0, 1, 0, 0]
    assert m.result()['episodes'] == 2 and m.result()['wins'] == [2, 0]


def test_run_by_episodes_reads_the_count_every_32_steps():
    m = Match(ScriptedEnv(), [_policy(0), _policy(1)])
    assert m.run(episodes=5, max_steps=100)['steps'] == 32
    m = Match(ScriptedEnv(), [_policy(0), _policy(1)])
    assert m.run(episodes=10 ** 6, max_steps=40)['steps'] == 40
    with pytest.raises(ValueError, match='max_steps'):
        m.run(episodes=5)
    with pytest.raises(ValueError):
        m.run()


def test_value_errors():
    with pytest.raises(ValueError, match='auto'):
        Match(ScriptedEnv(auto_reset=False), [_policy(0)])
    with pytest.raises(ValueError, match=r'12.*8|8.*12'):
        Match(ScriptedEnv(), [_policy(0), _policy(1, obs_dim=12)])
    with pytest.raises(ValueError, match='even'):
        Match(ScriptedEnv(n_envs=5), [_policy(0), _policy(1)], swap_sides=True)
    with pytest.raises(ValueError):
        Match(ScriptedEnv(), [_policy(0), _policy(1)], assignment=[0, 1, 0])
    with pytest.raises(ValueError):
        Match(ScriptedEnv(), [_policy(0)], assignment=[0, 1, 0, 1])


def test_load_policy_reads_a_bare_policy_file(tmp_path):
    p = _policy(3, obs_dim=11)
    path = tmp_path / 'bare.pt'
    torch.save({'policy': p.state_dict()}, path)
    q = load_policy(str(path), 'cpu')
    assert q.body[0].weight.shape == (256, 11)
    for (k, a), (_, b) in zip(p.state_dict().items(), q.state_dict().items()):
        assert torch.equal(a, b), k
    # a dict, with entries load_policy does not read
    r = load_policy({'policy': p.state_dict(), 'opt': object()})
    assert torch.equal(r.head.weight, p.head.weight)


def _history(greedy, seed):
    env = ScriptedEnv()
    Match(env, [_policy(0), _policy(1)], greedy=greedy, seed=seed).run(steps=6)
    return torch.stack(env.actions)


def test_greedy_match_does_not_depend_on_the_seed():
    g0, g1 = _history(True, 0), _history(True, 99)
    assert torch.equal(g0, g1)
    # each agent's greedy action is its own policy's per-head arg-max
    env = ScriptedEnv()
    obs = env.reset()
    pols = [_policy(0), _policy(1)]
    with torch.no_grad():
        for a in range(4):
            raw = pols[a // 2].forward_raw(obs[:, a])
            want = torch.stack([raw[:, o:o + n].argmax(-1) for o, n in
                                ((0, 3), (3, 3), (6, 3), (9, 2), (11, 2), (13, 2))], dim=-1)
            assert torch.equal(g0[0][:, a].long(), want)
    # the sampled match does depend on it, and is reproducible for one seed
    assert not torch.equal(_history(False, 0), _history(False, 99))
    assert torch.equal(_history(False, 5), _history(False, 5))
