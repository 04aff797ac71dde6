"""masurvival.match.Match on the GPU (C3 2v2, 64 envs, 40 steps) against
hand-written loops over the same kernels on a twin env with the same (seed, t)
keys, the greedy mode's independence of the seed, and the fp32 path of a
lidar config."""
import math

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.config import C3_CONFIG  # noqa: E402
from masurvival.match import Match  # noqa: E402
from masurvival.ppo import FusedPolicy, PolicyMLP  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

N, T = 64, 40


def _env(cfg=C3_CONFIG):
    return VecMaSurvival(cfg, n_envs=N, seeds=range(N), auto_reset=True)


def _policy(D, seed):
    torch.manual_seed(seed)
    return PolicyMLP(D).cuda()


class _Loop:
    """The hand-written side: bf16 rows from the reset, step_x after `act`."""

    def __init__(self, env, fp):
        self.env, A, D = env, env.n_agents, env.obs_dim
        M = N * A
        self.x = fp.x_buffer(M)
        self.x[:, :D].copy_(env.reset().reshape(M, D))
        self.a = torch.zeros((N, A, 6), dtype=torch.int8, device=env.device)
        self.lp = torch.empty((M,), device=env.device)
        self.v = torch.empty((M,), device=env.device)
        self.r = torch.empty((N, A), device=env.device)
        self.d = torch.empty((N,), dtype=torch.uint8, device=env.device)

    def step(self):
        self.env.step_x(self.a, self.x, self.r, self.d)


def test_one_policy_match_is_the_act_x_step_x_loop():
    env, twin = _env(), _env()
    assert env.supports_step_x()
    p = _policy(env.obs_dim, 1)
    m = Match(env, [p], seed=9)
    fp = FusedPolicy(p, env.obs_dim, env.device)
    fp.pack()
    lo = _Loop(twin, fp)
    for t in range(T):
        r, d = m.step()
        fp.act_x(lo.x, 9, t, lo.a.view(-1, 6), lo.lp, lo.v)
        lo.step()
        assert torch.equal(r, lo.r) and torch.equal(d, lo.d), t
        assert torch.equal(m.actions, lo.a), t
    assert torch.equal(env.get_state(), twin.get_state())
    assert m.result()['steps'] == T
    env.close()
    twin.close()


def test_two_policies_with_swapped_sides_is_the_act_sel_loop():
    env, twin = _env(), _env()
    D, A = env.obs_dim, env.n_agents
    p0, p1 = _policy(D, 2), _policy(D, 3)
    m = Match(env, [p0, p1], seed=4, swap_sides=True)
    res = m.run(steps=T)
    fps = [FusedPolicy(p, D, twin.device) for p in (p0, p1)]
    for fp in fps:
        fp.pack()
    lo = _Loop(twin, fps[0])
    a2 = lo.a.view(-1, 6)
    h = N // 2 * A
    ret = torch.zeros((N, A), dtype=torch.float64, device=twin.device)
    length = torch.zeros((N,), dtype=torch.int64, device=twin.device)
    wins, draws, eps, rsum, lsum = [0, 0], 0, 0, [0.0, 0.0], 0
    for t in range(T):
        # envs [0, N/2): agents 0, 1 -> policy 0, agents 2, 3 -> policy 1; the rest inverted
        fps[0].act_sel(lo.x[:h], A, 0b0011, 4, t, a2[:h], lo.lp[:h], lo.v[:h])
        fps[1].act_sel(lo.x[:h], A, 0b1100, 4, t, a2[:h], lo.lp[:h], lo.v[:h])
        fps[0].act_sel(lo.x[h:], A, 0b1100, 4, t, a2[h:], lo.lp[h:], lo.v[h:], first_row=h)
        fps[1].act_sel(lo.x[h:], A, 0b0011, 4, t, a2[h:], lo.lp[h:], lo.v[h:], first_row=h)
        lo.step()
        ret += lo.r
        length += 1
        for e in torch.nonzero(lo.d).flatten().tolist():
            front, back = float(ret[e, :2].sum()), float(ret[e, 2:].sum())
            s = (front, back) if e < N // 2 else (back, front)
            wins[0] += s[0] > s[1]
            wins[1] += s[1] > s[0]
            draws += s[0] == s[1]
            eps += 1
            rsum[0] += s[0]
            rsum[1] += s[1]
            lsum += int(length[e])
            ret[e] = 0
            length[e] = 0
    assert torch.equal(env.get_state(), twin.get_state())
    assert torch.equal(m.actions, lo.a)
    assert torch.equal(m._ret, ret)  # the unfinished episodes' running returns
    assert res['episodes'] == eps and res['wins'] == wins and res['draws'] == draws and res['steps'] == T
    assert res['return'] == pytest.approx([r / eps if eps else 0.0 for r in rsum], rel=1e-9)
    assert res['mean_length'] == pytest.approx(lsum / eps if eps else 0.0)
    env.close()
    twin.close()


def test_greedy_match_does_not_depend_on_the_seed():
    out = []
    for seed in (0, 12345):
        env = _env()
        D = env.obs_dim
        m = Match(env, [_policy(D, 5), _policy(D, 6)], greedy=True, seed=seed)
        out.append((m.run(steps=T), env.get_state().clone()))
        env.close()
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])


def test_lidar_config_plays_through_the_fp32_rows():
    lid = dict(C3_CONFIG, lidars={'n_lasers': 8, 'fov': 0.5 * math.pi, 'depth': 6})
    env = _env(lid)
    assert not env.supports_step_x()
    D = env.obs_dim
    m = Match(env, [_policy(D, 7), _policy(D, 8)], seed=1)
    assert not m.use_step_x
    for t in range(10):
        m.step()
        assert torch.equal(m.x[:, :D].view(torch.int16), env.obs.reshape(-1, D).bfloat16().view(torch.int16)), t
    assert bool((m.x[:, D] == 1).all())
    assert m.result()['steps'] == 10
    env.close()
