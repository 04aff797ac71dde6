"""PPOConfig.reward_norm on the fused x_obs path: 2v2 x 64 envs, horizon 8, two
minibatches.  What the trainer merges (every step's running return of the
rollout, before its GAE), the advantages it trains on (mas_gae over the scaled
copy, normalised), the checkpoint, the flag off against a config without the
flag, one self-play iteration and the one-rank all-reduce."""
import json
import os

import numpy as np
import pytest

import ret_ref as R

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import (PolicyMLP, PPOConfig, PPOTrainer, adv_normalize, gae,  # noqa: E402
                            scale_rewards_reference)
from masurvival.vec_env import VecMaSurvival  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'configs', '2v2.json')) as _f:
    CFG_2V2 = json.load(_f)
N, T, MB, A = 64, 8, 2, 4
F32 = np.float32


def _env(first_seed=0):
    return VecMaSurvival(CFG_2V2, n_envs=N, seeds=range(first_seed, first_seed + N), auto_reset=True)


def _cfg(**kw):
    return PPOConfig(horizon=T, minibatches=MB, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _params(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]).clone()


def _snapshot(tr):
    rn = tr.ret_norm
    return {'state': rn.state.clone(), 'carry': rn.carry.clone(), 'scale': rn.scale.clone(), 'params': _params(tr),
            'adv': tr.buf.adv.clone(), 'ret': tr.buf.ret.clone()}


def _check_against_records(tr, records, n_agents):
    """state, carry and scale against the restatement chained over the
    recorded raw rewards and dones (ret_ref.check_state: the tolerance of
    test_gpu_obs_norm_trainer.py's _check_state)."""
    M = records[0][0].shape[1]
    carry = np.zeros(M, dtype=F32)
    steps = []
    for r, d in records:
        s, carry, _ = R.ret_emulate(r, d, float(F32(tr.cfg.gamma)), carry, n_agents)
        steps.append(s)
    R.check_state(tr.ret_norm.state.cpu().numpy(), steps)
    got = tr.ret_norm.carry.cpu().numpy()
    assert np.array_equal(got.view(np.int32), carry.view(np.int32)), 'carry'
    want = R.scale_of(tr.ret_norm.state.cpu().numpy(), tr.cfg.reward_norm_eps)
    assert abs(float(tr.ret_norm.scale[0]) - float(want)) <= 2.0 ** -23 * float(want)  # the cast, and the double's last place


def _record(tr):
    b = tr.buf if tr.buf.learner is None else tr.buf.learner
    return b.rewards.reshape(T, -1).cpu().numpy().copy(), b.dones.cpu().numpy().copy()


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Two iterations with reward_norm on, a checkpoint, then a third:
    (trainer, records, snapshots after iterations 2 and 3, checkpoint path)."""
    env = _env()
    tr = PPOTrainer(env, _cfg(reward_norm=True), seed=0)
    assert tr.x_obs and tr.fused is not None
    assert tr.ret_norm.carry.shape == (N * A,) and float(tr.ret_norm.count) == 0
    records, stats = [], []
    for _ in range(2):
        tr.iteration()
        records.append(_record(tr))
        stats.append({k: float(v) for k, v in tr.last_stats.items()})
    _check_against_records(tr, records, A)
    snap2 = _snapshot(tr)
    raw = tr.buf.rewards.clone()
    # the advantages of iteration 2: mas_gae over the scaled copy, then mas_adv_normalize, bit for bit
    b = tr.buf
    copy = scale_rewards_reference(b.rewards, tr.ret_norm.scale, tr.cfg.reward_clip)
    adv, ret = torch.empty_like(b.adv), torch.empty_like(b.ret)
    st = torch.zeros((3,), dtype=torch.float64, device='cuda')
    gae(copy, b.values, b.dones, tr.cfg.gamma, tr.cfg.lam, adv, ret, st[:2], A)
    st[2] = float(adv.numel())
    adv_normalize(adv, st)
    replay = {'adv': adv, 'ret': ret, 'copy': copy, 'raw': raw}
    path = str(tmp_path_factory.mktemp('retnorm') / 'ckpt.pt')
    tr.save(path)
    tr.iteration()
    records.append(_record(tr))
    _check_against_records(tr, records, A)
    yield tr, records, stats, snap2, _snapshot(tr), replay, path
    env.close()


def test_state_and_carry_are_the_reference_over_the_recorded_rollouts(trained):
    tr, records, stats, snap2, snap3, _, _ = trained
    assert float(snap2['state'][0]) == 2 * T * N * A and float(snap3['state'][0]) == 3 * T * N * A
    for s in stats:
        assert all(np.isfinite(v) for v in s.values()), s
        assert 'reward_scale' in s and s['reward_scale'] > 0
    assert stats[1]['reward_scale'] == float(snap2['scale'][0])
    # the rewards the env wrote, not scaled ones: the 2v2 config's magnitudes survive in the buffer
    r = np.concatenate([x[0].reshape(-1) for x in records])
    assert np.isfinite(r).all() and np.abs(r).max() > 0


def test_advantages_are_mas_gae_over_the_scaled_copy_normalised(trained):
    _, _, _, snap2, _, replay, _ = trained
    assert torch.equal(_bits(snap2['ret']), _bits(replay['ret']))
    assert torch.equal(_bits(snap2['adv']), _bits(replay['adv']))
    assert not torch.equal(replay['copy'], replay['raw'])  # the scale was not 1: the check means something


def test_checkpoint_resumes_bitwise(trained):
    tr, _, _, snap2, snap3, _, path = trained
    sd = torch.load(path, map_location='cpu', weights_only=True)
    assert set(sd['ret_norm']) == {'count', 'mean', 'm2', 'eps', 'carry'}
    env = _env(first_seed=300)  # (the checkpoint brings the env state)
    tr2 = PPOTrainer(env, _cfg(reward_norm=True), seed=0)
    tr2.load(path)
    for k in ('state', 'carry', 'scale'):
        assert torch.equal(_bits(getattr(tr2.ret_norm, k)), _bits(snap2[k])), k
    tr2.iteration()
    got = _snapshot(tr2)
    for k in ('state', 'carry', 'scale', 'params', 'adv', 'ret'):
        assert torch.equal(_bits(got[k]), _bits(snap3[k])), k
    env.close()


def test_flag_off_is_the_config_without_the_flag():
    ea, eb = _env(), _env()
    a = PPOTrainer(ea, PPOConfig(horizon=T, minibatches=MB), seed=0)
    b = PPOTrainer(eb, _cfg(reward_norm=False, reward_clip=0.5, reward_norm_eps=1.0), seed=0)
    for _ in range(2):
        a.iteration()
        b.iteration()
    assert torch.equal(_bits(_params(a)), _bits(_params(b)))
    assert torch.equal(a.fused.packed, b.fused.packed) and torch.equal(_bits(a.buf.adv), _bits(b.buf.adv))
    assert b.ret_norm is None and 'ret_norm' not in b.state_dict() and 'reward_scale' not in b.last_stats
    ea.close()
    eb.close()


def test_self_play_carries_the_learners_columns():
    env = _env(first_seed=900)
    torch.manual_seed(11)
    sp = PPOTrainer(env, _cfg(reward_norm=True), seed=1, opponent=PolicyMLP(env.obs_dim), learner_agents=[0, 1])
    assert sp.ret_norm.carry.shape == (N * 2,)
    sp.iteration()
    lb = sp.buf.learner
    assert torch.equal(lb.rewards, sp.buf.rewards[:, :, :2])
    assert float(sp.ret_norm.count) == T * N * 2
    _check_against_records(sp, [_record(sp)], 2)
    assert all(bool(torch.isfinite(v)) for v in sp.last_stats.values())
    env.close()


def test_one_rank_allreduce_gives_the_state_without_it(trained, tmp_path):
    import torch.distributed as dist
    _, records, _, snap2, _, _, _ = trained
    assert not dist.is_initialized()
    dist.init_process_group('gloo', init_method=f'file://{tmp_path / "rdzv"}', rank=0, world_size=1)
    try:
        env = _env()
        tr = PPOTrainer(env, _cfg(reward_norm=True, allreduce=True), seed=0)
        assert tr.collectives and tr.world == 1
        recs = []
        for _ in range(2):
            tr.iteration()
            recs.append(_record(tr))
        _check_against_records(tr, recs, A)
        # a sum over one rank changes nothing: the same rollouts, the same bits
        for k in ('state', 'carry', 'scale'):
            assert torch.equal(_bits(getattr(tr.ret_norm, k)), _bits(snap2[k])), k
        for x, y in zip(recs, records):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        env.close()
    finally:
        dist.destroy_process_group()
