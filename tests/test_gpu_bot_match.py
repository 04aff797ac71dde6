"""Scripted bots in Match and in the self-play trainer on the GPU (C3 2v2):
a Match with a policy and a bot against the hand-written act_sel + mas_bot_act
+ step_x loop, the hunter against the idle bot over 256 episodes, and
PPOTrainer(opponent='bot:hunter'): the opponent's rows against tests/bot_ref.py,
the learner's rows against a trainer with a policy opponent, and the
checkpoint round trip."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import bot_ref  # noqa: E402
from masurvival.bots import BOT_KINDS, bot_act  # noqa: E402
from masurvival.config import C3_CONFIG  # noqa: E402
from masurvival.match import Match  # noqa: E402
from masurvival.ppo import FusedPolicy, PolicyMLP, PPOConfig, PPOTrainer  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

N, T = 64, 64


def _env(n=N):
    return VecMaSurvival(C3_CONFIG, n_envs=n, seeds=range(n), auto_reset=True)


def test_match_with_a_bot_is_the_act_sel_bot_act_step_x_loop():
    env, twin = _env(), _env()
    D, A = env.obs_dim, env.n_agents
    torch.manual_seed(2)
    p = PolicyMLP(D).cuda()
    m = Match(env, [p, 'bot:hunter'], seed=4, swap_sides=True)
    fp = FusedPolicy(p, D, twin.device)
    fp.pack()
    cs = twin.rc.to_struct()
    M, h = N * A, N // 2 * A
    x = fp.x_buffer(M)
    x[:, :D].copy_(twin.reset().reshape(M, D))
    a = torch.zeros((N, A, 6), dtype=torch.int8, device=twin.device)
    a2 = a.view(-1, 6)
    lp, v = torch.empty((M,), device=twin.device), torch.empty((M,), device=twin.device)
    r = torch.empty((N, A), device=twin.device)
    d = torch.empty((N,), dtype=torch.uint8, device=twin.device)
    for t in range(T):
        mr, md = m.step()
        # envs [0, N/2): agents 0, 1 -> the policy, agents 2, 3 -> the bot; the rest inverted
        fp.act_sel(x[:h], A, 0b0011, 4, t, a2[:h], lp[:h], v[:h])
        bot_act(cs, 'hunter', x[:h], A, 0b1100, a2[:h])
        fp.act_sel(x[h:], A, 0b1100, 4, t, a2[h:], lp[h:], v[h:], first_row=h)
        bot_act(cs, 'hunter', x[h:], A, 0b0011, a2[h:])
        twin.step_x(a, x, r, d)
        assert torch.equal(m.actions, a), t
        assert torch.equal(mr, r) and torch.equal(md, d), t
    assert torch.equal(env.get_state(), twin.get_state())
    assert torch.equal(m.x, x)
    env.close()
    twin.close()


def test_hunter_beats_idle_over_256_episodes():
    env = _env(256)
    m = Match(env, ['bot:hunter', 'bot:idle'], swap_sides=True)
    res = m.run(episodes=256, max_steps=6000)
    env.close()
    assert res['episodes'] >= 256, res
    assert res['wins'][0] > res['wins'][1], res


TT, MB, LA = 16, 2, [0, 1]


def _trainer(opponent):
    return PPOTrainer(_env(), PPOConfig(horizon=TT, minibatches=MB), seed=0, opponent=opponent, learner_agents=LA)


def test_trainer_with_a_bot_opponent(tmp_path):
    tr = _trainer('bot:hunter')
    assert tr.opponent is None and tr.opp_fused is None and tr.opponent_bot.name == 'hunter'
    torch.manual_seed(77)
    pol = _trainer(PolicyMLP(tr.env.obs_dim, 256))
    cs, b, A = tr.env.rc.to_struct(), tr.buf, tr.buf.A
    opp = np.tile(np.array([False, False, True, True]), N)
    for it in range(2):
        for t in range(TT):
            tr.rollout_step(t)
        if it == 0:
            # the learner's rows do not depend on what fills the other rows at step 0
            pol.rollout_step(0)
            la = ~torch.from_numpy(opp).cuda()
            assert torch.equal(b.actions[0].view(-1, 6)[la], pol.buf.actions[0].view(-1, 6)[la])
            assert torch.equal(b.logp[0].view(-1)[la], pol.buf.logp[0].view(-1)[la])
            assert torch.equal(b.values[0].view(-1)[la], pol.buf.values[0].view(-1)[la])
        rows = b.xb[:TT].float().cpu().numpy().reshape(TT * N * A, -1)
        got = b.actions.cpu().numpy().reshape(TT * N * A, 6)
        want, near = bot_ref.bot_ref(BOT_KINDS['hunter'], rows, cs)
        sel = np.tile(opp, TT)
        bad = (got != want).any(axis=1) & sel & ~near
        assert not bad.any(), f'iteration {it}: {int(bad.sum())} opponent rows differ ({int((near & sel).sum())} near)'
        assert int((near & sel).sum()) <= 0.005 * int(sel.sum())
        tr.finish_rollout()
        tr.update()
    # save and load reproduce the next iteration bit for bit
    path = str(tmp_path / 'bot.pt')
    tr.save(path)
    sd = torch.load(path, map_location='cpu', weights_only=True)
    assert sd['opponent_bot'] == 'hunter' and 'opponent' not in sd
    twin = _trainer('bot:hunter')
    twin.load(path)
    tr.iteration()
    twin.iteration()
    torch.cuda.synchronize()
    for p, q in zip(tr.policy.parameters(), twin.policy.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(tr.buf.actions, twin.buf.actions)
    with pytest.raises(ValueError, match='opponent bot'):
        _trainer('bot:forager').load(path)
    with pytest.raises(ValueError, match='bot'):
        tr.sync_opponent()
    for t_ in (tr, twin, pol):
        t_.env.close()
