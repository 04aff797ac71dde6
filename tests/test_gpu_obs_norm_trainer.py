"""PPOConfig.obs_norm on the fused x_obs path: 2v2 x 64 envs, horizon 8, two
minibatches.  What the trainer merges and when (the reset rows, then blocks
[0, T) of each rollout after its update), the checkpoint through Match, the
flag off against a config without the flag, and one self-play iteration
against a checkpoint that carries its own normaliser."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.match import Match, load_policy  # noqa: E402
from masurvival.ppo import PPOConfig, PPOTrainer  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'configs', '2v2.json')) as _f:
    CFG_2V2 = json.load(_f)
N, T, MB = 64, 8, 2


def _env(first_seed=0):
    return VecMaSurvival(CFG_2V2, n_envs=N, seeds=range(first_seed, first_seed + N), auto_reset=True)


def _cfg(**kw):
    return PPOConfig(horizon=T, minibatches=MB, **kw)


def _check_state(state, blocks, D):
    """state (count, mean, m2) against the two-pass fp64 moments of all merged
    rows.  The kernel's sums are within n 2^-52 sum|term| of exact
    (tests/test_gpu_obs_stats.py) and m2 comes from sum x^2 - n mean^2 plus a
    few fp64 roundings per merge, each far below one of those: eight times
    that bound for both."""
    x = np.concatenate([b.reshape(-1, b.shape[-1])[:, :D].float().double().cpu().numpy() for b in blocks])
    n = x.shape[0]
    got = state.cpu().numpy()
    assert got[0] == n
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    tol = 8 * n * 2.0 ** -52
    assert (np.abs(got[1:1 + D] - mean) <= tol * np.abs(x).sum(0) / n + 1e-300).all()
    assert (np.abs(got[1 + D:] - m2) <= tol * (x * x).sum(0) + 1e-300).all()


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Two iterations with obs_norm on; (trainer, the blocks it merged, checkpoint path)."""
    env = _env()
    tr = PPOTrainer(env, _cfg(obs_norm=True), seed=0)
    assert tr.x_obs and tr.fused is not None
    D = env.obs_dim
    blocks = [tr.buf.xb[0].clone()]  # the reset rows
    _check_state(tr.obs_norm.state, blocks, D)
    stats = []
    for _ in range(2):
        first = tr.buf.xb[0].clone()  # (block 0 is overwritten by the next rollout's first rows)
        tr.iteration()
        blocks += [first, tr.buf.xb[1:T].clone()]
        stats.append({k: float(v) for k, v in tr.last_stats.items()})
    path = str(tmp_path_factory.mktemp('obsnorm') / 'ckpt.pt')
    tr.save(path)
    yield tr, blocks, stats, path
    env.close()


def test_state_is_the_moments_of_the_merged_blocks(trained):
    tr, blocks, stats, _ = trained
    D = tr.env.obs_dim
    _check_state(tr.obs_norm.state, blocks, D)
    assert float(tr.obs_norm.count) == N * 4 * (1 + 2 * T)
    for s in stats:
        assert all(np.isfinite(v) for v in s.values()), s
    on = tr.obs_norm
    assert tr.policy.obs_mean is on.mean and tr.policy.obs_inv_std is on.inv_std
    assert bool(torch.isfinite(on.mean).all()) and float(on.inv_std.max()) <= 10.0 and float(on.inv_std.min()) > 0


def test_checkpoint_plays_a_match_with_the_trainers_packed_image(trained):
    tr, _, _, path = trained
    sd = torch.load(path, map_location='cpu', weights_only=True)
    assert set(sd['obs_norm']) == {'count', 'mean', 'm2', 'eps'}
    pol = load_policy(path, 'cuda')
    assert torch.equal(pol.obs_mean, tr.obs_norm.mean) and torch.equal(pol.obs_inv_std, tr.obs_norm.inv_std)
    menv = _env(first_seed=500)
    m = Match(menv, [pol], seed=1)
    res = m.run(steps=16)
    assert res['steps'] == 16
    fp = m.actor.fused[0]
    assert torch.equal(fp.packed, tr.fused.packed)
    # the same rows through both packed policies: the same bits
    x = tr.buf.xb[0]
    M = x.shape[0]
    outs = []
    for f in (fp, tr.fused):
        acts = torch.zeros((M, 6), dtype=torch.int8, device='cuda')
        lp, v = torch.zeros((M,), device='cuda'), torch.zeros((M,), device='cuda')
        lg = torch.zeros((M, 16), device='cuda')
        f.act_sel(x, 4, 0b1111, 3, 7, acts, lp, v, logits=lg)
        outs.append((acts, lp, v, lg))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][3]).all())
    menv.close()


def test_flag_off_is_the_config_without_the_flag():
    ea, eb = _env(), _env()
    a = PPOTrainer(ea, PPOConfig(horizon=T, minibatches=MB), seed=0)
    b = PPOTrainer(eb, _cfg(obs_norm=False), seed=0)
    a.iteration()
    b.iteration()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(a.fused.packed, b.fused.packed) and torch.equal(a.buf.xb, b.buf.xb)
    assert b.obs_norm is None and 'obs_norm' not in b.state_dict()
    ea.close()
    eb.close()


def test_self_play_against_a_checkpoint_with_its_own_normaliser(trained):
    tr, _, _, path = trained
    env = _env(first_seed=900)
    sp = PPOTrainer(env, _cfg(obs_norm=True), seed=1, opponent=path, learner_agents=[0, 1])
    assert torch.equal(sp.opponent.obs_mean, tr.obs_norm.mean)
    assert float(sp.obs_norm.count) == N * 2  # the learner's reset rows
    opp_image = sp.opp_fused.packed.clone()
    learner_before = sp.fused.packed.clone()
    sp.iteration()
    assert float(sp.obs_norm.count) == N * 2 * (1 + T)
    _check_state(sp.obs_norm.state, [sp.buf.learner.xb[0], sp.buf.learner.xb], env.obs_dim)
    assert all(bool(torch.isfinite(v)) for v in sp.last_stats.values())
    # the opponent keeps its own frozen statistics, the learner's have moved
    assert torch.equal(sp.opp_fused.packed, opp_image) and torch.equal(sp.opponent.obs_mean, tr.obs_norm.mean)
    assert not torch.equal(sp.fused.packed, learner_before) and not torch.equal(sp.fused.packed, sp.opp_fused.packed)
    assert not torch.equal(sp.policy.obs_mean, sp.opponent.obs_mean)
    # both acted: every agent's actions are in range and neither side's are all one value
    acts = sp.buf.actions.long()
    hi = torch.tensor([3, 3, 3, 2, 2, 2], device='cuda')
    assert bool(((acts >= 0) & (acts < hi)).all())
    for side in ([0, 1], [2, 3]):
        assert int(acts[:, :, side].reshape(-1, 6)[:, 0].unique().numel()) > 1
    env.close()
