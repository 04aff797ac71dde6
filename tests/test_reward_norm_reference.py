"""Running return normalisation of the rewards, host side (no GPU): the torch
restatement of mas_ret_stats held to the fp64 recurrence of tests/ret_ref.py
within its derived bound (and the checker to its mutations), the merge through
merge_reference with one column, the invariance of the scaled rewards under a
power-of-two rescaling, and the trainer on the CPU stand-in env of
tests/test_ppo.py (restated here): what it merges and when, the raw rewards
buffer, checkpoints, the flag off, two gloo ranks."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ret_ref as R
from masurvival.ppo import (PPOConfig, PPOTrainer, RetNorm, gae_reference_into, merge_reference, ret_stats_reference,
                            scale_rewards_reference)

F32 = np.float32
GAMMA = float(F32(0.99))
T_H = 6  # the trainers' horizon


class StandInEnv:
    """Deterministic CPU env with VecMaSurvival's step/reset surface (the test
    double of tests/test_ppo.py); `reward_scale` multiplies every reward."""

    def __init__(self, n_envs=8, n_agents=4, obs_dim=12, seed=0, reward_scale=1.0):
        self.n_envs, self.n_agents, self.obs_dim = n_envs, n_agents, obs_dim
        self.device = torch.device('cpu')
        self.g = torch.Generator().manual_seed(seed)
        self.t = 0
        self.reward_scale = float(reward_scale)

    def reset(self):
        return torch.randn((self.n_envs, self.n_agents, self.obs_dim), generator=self.g)

    def step(self, actions, out=None):
        self.t += 1
        o, r, d = out
        o.copy_(torch.randn(o.shape, generator=self.g))
        r.copy_(((actions[..., 0].float() - 1.0) * 0.5 + (actions[..., 3].float())) * self.reward_scale)
        d.copy_(((torch.arange(self.n_envs) + self.t) % 5 == 0).to(torch.uint8))
        return o, r, d, {}

    def get_state(self):
        return torch.cat([self.g.get_state(), torch.tensor([self.t], dtype=torch.int64).view(torch.uint8)])

    def set_state(self, buf):
        self.g.set_state(buf[:-8].clone())
        self.t = int(buf[-8:].clone().view(torch.int64)[0])


def _data(T=17, E=43, A=3, p_done=0.1, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((T, E * A)) * scale).astype(F32)
    d = (rng.random((T, E)) < p_done).astype(np.uint8)
    d[d != 0] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=int((d != 0).sum()))
    carry = (rng.standard_normal(E * A) * 3 * scale).astype(F32)
    return r, d, carry


def _reference(r, d, carry, A, gamma=GAMMA):
    steps = torch.empty(r.shape, dtype=torch.float32)
    new, sums = ret_stats_reference(torch.from_numpy(r), torch.from_numpy(d), gamma, torch.from_numpy(carry), A,
                                    steps_out=steps)
    return steps.numpy(), new.numpy(), sums.numpy()


def test_restatement_is_within_the_derived_bound_of_the_fp64_recurrence():
    r, d, carry = _data()
    keep = carry.copy()
    steps, new, sums = _reference(r, d, carry, 3)
    assert np.array_equal(carry, keep), 'the carry going in was written'
    q = R.check_steps(r, d, GAMMA, carry, 3, steps)
    print(f'worst |R - ref| / bound: {q:.3f}')
    assert 0.0 < q <= 1.0, q
    # the carry out is the last step's return, 0 where that step was done
    dcol = np.repeat(d[-1] != 0, 3)
    assert np.array_equal(new, np.where(dcol, F32(0), steps[-1]))
    # bit for bit the emulation of the kernel's arithmetic
    e_steps, e_carry, _ = R.ret_emulate(r, d, GAMMA, carry, 3)
    assert np.array_equal(steps.view(np.int32), e_steps.view(np.int32))
    assert np.array_equal(new.view(np.int32), e_carry.view(np.int32))
    assert max(R.check_sums(sums, steps)) <= 1.0
    assert sums.dtype == np.float64 and new.dtype == np.float32


@pytest.mark.parametrize('gamma', [0.0, 1.0, float(F32(0.999))])
def test_restatement_at_other_discounts(gamma):
    r, d, carry = _data(T=9, E=5, A=2, seed=3)
    steps, _, sums = _reference(r, d, carry, 2, gamma)
    assert R.check_steps(r, d, gamma, carry, 2, steps) <= 1.0
    assert max(R.check_sums(sums, steps)) <= 1.0
    if gamma == 0.0:
        assert np.array_equal(steps, r)


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_the_checker_catches_each_mutation(mut):
    r, d, carry = _data()
    good, _, _ = R.ret_emulate(r, d, GAMMA, carry, 3)
    assert R.check_steps(r, d, GAMMA, carry, 3, good) <= 1.0
    bad, _, _ = R.ret_emulate(r, d, GAMMA, carry, 3, mut)
    q = R.check_steps(r, d, GAMMA, carry, 3, bad)
    assert q > 1.0, (mut, q)


def test_three_updates_merge_to_the_moments_of_all_returns():
    """RetNorm on the CPU: ret_stats_reference + merge_reference with one column."""
    A, E = 3, 7
    rn = RetNorm(E * A, 'cpu', eps=1e-8)
    assert rn.state.dtype == torch.float64 and rn.state.shape == (3,) and rn.batch.shape == (3,)
    assert rn.carry.dtype == torch.float32 and rn.carry.shape == (E * A,) and not rn.carry.any()
    assert rn.scale.dtype == torch.float32 and rn.scale.tolist() == [1.0]
    ref_state = torch.zeros((3,), dtype=torch.float64)
    carry = np.zeros(E * A, dtype=F32)
    all_steps = []
    for k, T in enumerate((5, 1, 12)):
        r, d, _ = _data(T=T, E=E, A=A, seed=10 + k)
        tr, td = torch.from_numpy(r), torch.from_numpy(d)
        keep = tr.clone()
        rn.update(tr.view(T, E, A), td, A, GAMMA)
        assert torch.equal(tr, keep)
        steps, carry, sums = R.ret_emulate(r, d, GAMMA, carry, A)
        all_steps.append(steps)
        batch = torch.tensor([float(T * E * A), sums[0], sums[1]], dtype=torch.float64)
        _, want_scale = merge_reference(ref_state, batch, 1e-8)
        assert np.array_equal(rn.carry.numpy().view(np.int32), carry.view(np.int32))
        torch.testing.assert_close(rn.state, ref_state, rtol=1e-13, atol=0)
        torch.testing.assert_close(rn.scale, want_scale, rtol=2e-7, atol=0)
    R.check_state(rn.state.numpy(), all_steps)
    n, mean, m2 = R.moments(all_steps)
    assert abs(float(rn.scale[0]) - 1.0 / math.sqrt(m2 / n + 1e-8)) <= 2e-7 * float(rn.scale[0])
    # the state round-trips, the carry's shape is checked
    back = RetNorm.from_state_dict(rn.state_dict(), 'cpu')
    assert torch.equal(back.state, rn.state) and torch.equal(back.carry, rn.carry) and torch.equal(back.scale, rn.scale)
    assert set(rn.state_dict()) == {'count', 'mean', 'm2', 'eps', 'carry'}
    with pytest.raises(ValueError):
        RetNorm(E * A + 1, 'cpu').load_state_dict(rn.state_dict())
    with pytest.raises(ValueError):
        rn.update(torch.zeros((4, E + 1, A)), torch.zeros((4, E + 1), dtype=torch.uint8), A, GAMMA)


def test_scaled_rewards_are_invariant_under_a_power_of_two():
    """eps = 0, no clip: rewards x 4 give R x 4, sums x 4 and x 16, a state
    (mean x 4, m2 x 16) and a scale / 4, every step exact in binary floating
    point, so the scaled rewards are the same bits over three updates."""
    A, E = 2, 9
    a, b = RetNorm(E * A, 'cpu', eps=0.0), RetNorm(E * A, 'cpu', eps=0.0)
    for k, T in enumerate((6, 3, 11)):
        r, d, _ = _data(T=T, E=E, A=A, seed=20 + k)
        ra, rb = torch.from_numpy(r), torch.from_numpy(r * F32(4))
        td = torch.from_numpy(d)
        a.update(ra, td, A, GAMMA)
        b.update(rb, td, A, GAMMA)
        assert float(b.scale[0]) * 4 == float(a.scale[0])
        sa = scale_rewards_reference(ra, a.scale, math.inf)
        sb = scale_rewards_reference(rb, b.scale, math.inf)
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)), k
        assert torch.equal(b.carry, a.carry * 4)
    assert float(b.state[1]) == 4 * float(a.state[1]) and float(b.state[2]) == 16 * float(a.state[2])


def test_scaling_restatement_rounds_the_product_then_clamps_and_passes_nan():
    r = torch.tensor([0.1, -0.1, 3.0, -3.0, 5.0, -7.0, float('nan'), float('inf'), -float('inf'), 0.0])
    s = torch.tensor([0.37])
    out = scale_rewards_reference(r, s, 1.5)
    want = np.clip(r.numpy() * F32(0.37), F32(-1.5), F32(1.5))
    assert np.array_equal(out.numpy()[:6], want[:6]) and math.isnan(float(out[6]))
    assert out.tolist()[7:] == [1.5, -1.5, 0.0]
    assert out[2] == F32(3.0) * F32(0.37) and out[4] == 1.5 and out[5] == -1.5
    assert r[2] == 3.0  # a copy


def _trainer(env, **kw):
    cfg = PPOConfig(horizon=T_H, hidden=32, minibatches=2, autocast_bf16=False, **kw)
    tr = PPOTrainer(env, cfg, seed=3)
    tr.gae_impl = gae_reference_into
    return tr


def _recorded_iteration(tr):
    """One iteration; (raw rewards, dones) of its rollout as numpy copies."""
    tr.iteration()
    b = tr.buf
    return b.rewards.reshape(T_H, -1).numpy().copy(), b.dones.numpy().copy()


def test_cpu_trainer_state_is_the_moments_of_the_recomputed_returns():
    env = StandInEnv()
    tr = _trainer(env, reward_norm=True)
    A, M = env.n_agents, env.n_envs * env.n_agents
    assert tr.ret_norm.carry.shape == (M,) and float(tr.ret_norm.count) == 0
    carry = np.zeros(M, dtype=F32)
    steps_all = []
    for it in range(3):
        scale_before = tr.ret_norm.scale.clone()
        r, d = _recorded_iteration(tr)
        steps, carry, _ = R.ret_emulate(r, d, float(F32(tr.cfg.gamma)), carry, A)
        steps_all.append(steps)
        R.check_state(tr.ret_norm.state.numpy(), steps_all)
        assert np.array_equal(tr.ret_norm.carry.numpy().view(np.int32), carry.view(np.int32)), it
        want = R.scale_of(tr.ret_norm.state.numpy(), tr.cfg.reward_norm_eps)
        assert abs(float(tr.ret_norm.scale[0]) - float(want)) <= 2e-7 * float(want)
        assert not torch.equal(tr.ret_norm.scale, scale_before)  # merged before this rollout's GAE read it
        assert float(tr.last_stats['reward_scale']) == float(tr.ret_norm.scale[0])
        # the buffer keeps the raw rewards: the stand-in env's six values
        assert set(np.unique(r).tolist()) <= {-0.5, 0.0, 0.5, 1.0, 1.5}
        # the value targets were built from the scaled rewards
        adv = torch.empty_like(tr.buf.adv)
        ret = torch.empty_like(tr.buf.ret)
        sums = torch.zeros((2,), dtype=torch.float64)
        scaled = scale_rewards_reference(tr.buf.rewards, tr.ret_norm.scale, tr.cfg.reward_clip)
        gae_reference_into(scaled, tr.buf.values, tr.buf.dones, tr.cfg.gamma, tr.cfg.lam, adv, ret, sums, A)
        assert torch.equal(ret, tr.buf.ret)
    assert float(tr.ret_norm.count) == 3 * T_H * M
    assert torch.isfinite(tr.last_stats['loss'])


def test_first_iteration_already_has_statistics_and_the_clip_bites():
    env = StandInEnv(reward_scale=100.0)
    tr = _trainer(env, reward_norm=True, reward_clip=0.5)
    tr.iteration()
    assert float(tr.ret_norm.count) == T_H * 32 and float(tr.ret_norm.scale[0]) < 0.05  # returns of order 100
    scaled = scale_rewards_reference(tr.buf.rewards, tr.ret_norm.scale, 0.5)
    assert float(scaled.abs().max()) == 0.5 and float(tr.buf.rewards.abs().max()) == 150.0
    with pytest.raises(ValueError):
        _trainer(StandInEnv(), reward_norm=True, reward_clip=0.0)


def test_checkpoint_round_trip_continues_with_identical_parameters_and_state(tmp_path):
    tr = _trainer(StandInEnv(), reward_norm=True)
    tr.iteration()
    path = str(tmp_path / 'ckpt.pt')
    tr.save(path)
    sd = torch.load(path, weights_only=True)
    assert set(sd['ret_norm']) == {'count', 'mean', 'm2', 'eps', 'carry'}
    assert all(sd['ret_norm'][k].dtype == torch.float64 for k in ('count', 'mean', 'm2'))
    assert sd['ret_norm']['carry'].dtype == torch.float32
    tr.iteration()
    tr2 = _trainer(StandInEnv(seed=99), reward_norm=True)
    tr2.load(path)
    tr2.iteration()
    assert torch.equal(tr.ret_norm.state, tr2.ret_norm.state) and torch.equal(tr.ret_norm.carry, tr2.ret_norm.carry)
    assert torch.equal(tr.ret_norm.scale, tr2.ret_norm.scale)
    for a, b in zip(tr.policy.parameters(), tr2.policy.parameters()):
        assert torch.equal(a, b)
    # the flag off: the checkpoint's statistics are restored and applied, not updated
    tr3 = _trainer(StandInEnv(seed=5))
    assert tr3.ret_norm is None and 'ret_norm' not in tr3.state_dict()
    tr3.load(path)
    assert torch.equal(tr3.ret_norm.state, torch.stack([sd['ret_norm'][k] for k in ('count', 'mean', 'm2')]))
    frozen, carry = tr3.ret_norm.state.clone(), tr3.ret_norm.carry.clone()
    tr3.iteration()
    assert torch.equal(tr3.ret_norm.state, frozen) and torch.equal(tr3.ret_norm.carry, carry)
    assert 'ret_norm' in tr3.state_dict() and 'reward_scale' not in tr3.last_stats
    # a carry of another shape is refused
    with pytest.raises(ValueError):
        _trainer(StandInEnv(n_envs=4), reward_norm=True).load_state_dict(sd)


def test_checkpoint_without_the_key_loads_into_a_flagged_trainer_that_starts_fresh(tmp_path):
    tr = _trainer(StandInEnv())
    tr.iteration()
    assert 'ret_norm' not in tr.state_dict()
    path = str(tmp_path / 'old.pt')
    tr.save(path)
    tr2 = _trainer(StandInEnv(seed=1), reward_norm=True)
    tr2.load(path)
    assert float(tr2.ret_norm.count) == 0 and tr2.ret_norm.scale.tolist() == [1.0]
    tr2.iteration()
    assert float(tr2.ret_norm.count) == T_H * 32 and torch.isfinite(tr2.last_stats['loss'])


def test_flag_off_is_the_trainer_without_the_flag():
    a = PPOTrainer(StandInEnv(), PPOConfig(horizon=T_H, hidden=32, minibatches=2, autocast_bf16=False), seed=3)
    b = _trainer(StandInEnv(), reward_norm=False, reward_clip=0.125, reward_norm_eps=0.5)
    on = _trainer(StandInEnv(), reward_norm=True)
    a.gae_impl = gae_reference_into
    for tr in (a, b, on):
        tr.iteration()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(a.buf.adv, b.buf.adv) and torch.equal(a.buf.ret, b.buf.ret)
    assert b.ret_norm is None and 'reward_scale' not in b.last_stats
    assert not torch.equal(a.buf.ret, on.buf.ret)  # and the flag on is another trainer
    cfg = PPOConfig()
    assert (cfg.reward_norm, cfg.reward_norm_eps, cfg.reward_clip) == (False, 1e-8, 10.0)


def test_self_play_carries_the_learners_columns():
    from masurvival.ppo import PolicyMLP
    env = StandInEnv()
    tr = PPOTrainer(env, PPOConfig(horizon=T_H, hidden=32, minibatches=2, autocast_bf16=False, reward_norm=True),
                    seed=3, opponent=PolicyMLP(env.obs_dim, 32), learner_agents=[0, 2])
    tr.gae_impl = gae_reference_into
    assert tr.ret_norm.carry.shape == (env.n_envs * 2,)
    tr.iteration()
    lb = tr.buf.learner
    assert torch.equal(lb.rewards, tr.buf.rewards[:, :, [0, 2]])
    steps, carry, _ = R.ret_emulate(lb.rewards.reshape(T_H, -1).numpy(), lb.dones.numpy(), float(F32(tr.cfg.gamma)),
                                    np.zeros(env.n_envs * 2, dtype=F32), 2)
    R.check_state(tr.ret_norm.state.numpy(), [steps])
    assert np.array_equal(tr.ret_norm.carry.numpy(), carry)


def _rank_main(rank, world, init_file, out_dir):
    dist.init_process_group('gloo', init_method=f'file://{init_file}', rank=rank, world_size=world)
    torch.set_num_threads(1)
    tr = _trainer(StandInEnv(seed=100 + rank), reward_norm=True)
    rec = []
    for _ in range(2):
        rec.append(_recorded_iteration(tr))
    flat = torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()])
    torch.save({'flat': flat, 'state': tr.ret_norm.state, 'scale': tr.ret_norm.scale, 'carry': tr.ret_norm.carry,
                'rewards': torch.from_numpy(np.stack([r for r, _ in rec])),
                'dones': torch.from_numpy(np.stack([d for _, d in rec]))}, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_gloo_state_is_identical_and_that_of_one_process_over_both_shards(tmp_path):
    ctx = mp.get_context('spawn')
    init_file = str(tmp_path / 'rdzv')
    ps = [ctx.Process(target=_rank_main, args=(r, 2, init_file, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(150)
        assert p.exitcode == 0
    res = [torch.load(str(tmp_path / f'rank{r}.pt'), weights_only=True) for r in range(2)]
    assert not torch.equal(res[0]['rewards'], res[1]['rewards'])  # the ranks saw different rewards
    for k in ('state', 'scale', 'flat'):
        assert torch.equal(res[0][k], res[1][k]), k
    assert float(res[0]['state'][0]) == 2 * 2 * T_H * 32  # the counts are global
    # one process over both shards: the ranks' columns side by side
    one = RetNorm(2 * 32, 'cpu')
    for it in range(2):
        r = torch.cat([res[k]['rewards'][it].view(T_H, 8, 4) for k in range(2)], dim=1)
        d = torch.cat([res[k]['dones'][it] for k in range(2)], dim=1)
        one.update(r.contiguous(), d.contiguous(), 4, 0.99)
    torch.testing.assert_close(res[0]['state'], one.state, rtol=1e-13, atol=0)
    torch.testing.assert_close(res[0]['scale'], one.scale, rtol=2e-7, atol=0)
    assert torch.equal(torch.cat([res[0]['carry'].view(8, 4), res[1]['carry'].view(8, 4)]).view(-1), one.carry)
