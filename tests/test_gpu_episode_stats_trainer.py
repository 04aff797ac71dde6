"""PPOConfig.episode_stats on the fused x_obs path: 2v2 x 64 envs, horizon 16,
two minibatches, four iterations, with and without a frozen opponent.  What the
trainer totals (the restatement of tests/ep_ref.py chained over clones of every
rollout's rewards and dones), that the feature only reads (the parameters with
the flag on are those with it off, bit for bit), and the checkpoint.

The stock 2v2 config's episodes outlast these rollouts (300 steps of immunity,
a zone that closes every 100 steps), so the config below shortens them: two
steps of immunity, a zone phase every three steps, zone damage of a whole
health bar.  By the CPU oracle under random actions its episodes last 6 to 19
steps, with wins of both sides and draws."""
import json
import os

import numpy as np
import pytest

import ep_ref as R

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import PolicyMLP, PPOConfig, PPOTrainer  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'configs', '2v2.json')) as _f:
    CFG_SHORT = json.load(_f)
CFG_SHORT['immunity_phase'] = {'cooldown': 2}
CFG_SHORT['safe_zone'] = {'cooldown': 3, 'damage': 100}  # (merged over the default phases and radii)
N, T, MB, A, ITERS = 64, 16, 2, 4, 4
EP_KEYS = ('episodes', 'ep_length', 'ep_return', 'win_rate')


def _env(first_seed=0):
    return VecMaSurvival(CFG_SHORT, n_envs=N, seeds=range(first_seed, first_seed + N), auto_reset=True)


def _trainer(env, selfplay, **kw):
    cfg = PPOConfig(horizon=T, minibatches=MB, **kw)
    if not selfplay:
        return PPOTrainer(env, cfg, seed=0)
    torch.manual_seed(11)
    return PPOTrainer(env, cfg, seed=0, opponent=PolicyMLP(env.obs_dim), learner_agents=[0, 1])


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _params(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]).clone()


def _state(tr):
    es = tr.ep_stats
    return {k: getattr(es, k).clone() for k in ('total', 'last', 'ret_carry', 'len_carry')}


@pytest.fixture(scope='module', params=[False, True], ids=['shared', 'selfplay'])
def trained(request, tmp_path_factory):
    """Four iterations with the flag on, a checkpoint after the second:
    (selfplay, trainer, per-iteration clones of the whole buffer's rewards and
    dones, per-iteration last_stats, state after iterations 2 and 4, parameters, path)."""
    selfplay = request.param
    env = _env()
    tr = _trainer(env, selfplay, episode_stats=True)
    assert tr.x_obs and tr.fused is not None
    assert tr.ep_stats.side_mask == 0b0011 and (tr.ep_stats.n_envs, tr.ep_stats.n_agents) == (N, A)
    records, stats = [], []
    path = str(tmp_path_factory.mktemp('epstats') / 'ckpt.pt')
    for it in range(ITERS):
        tr.iteration()
        records.append((tr.buf.rewards.reshape(T, -1).cpu().numpy().copy(), tr.buf.dones.cpu().numpy().copy()))
        assert all(isinstance(tr.last_stats[k], torch.Tensor) and tr.last_stats[k].is_cuda for k in EP_KEYS)
        stats.append({k: tr.last_stats[k].tolist() for k in EP_KEYS})
        if it == 1:
            tr.save(path)
            state2 = _state(tr)
    yield selfplay, tr, records, stats, state2, _state(tr), _params(tr), path
    env.close()


def test_totals_are_the_restatement_chained_over_the_recorded_rollouts(trained):
    _, tr, records, stats, _, state4, _, _ = trained
    G, ln = [0.0] * (N * A), [0] * N
    total = dict.fromkeys(R.HEAD, 0)
    eps = [[] for _ in range(A)]
    for (r, d), ls in zip(records, stats):
        G, ln, c, ep = R.walk(r, d, A, G, ln, 0b0011)
        n = c['episodes']
        total = {k: total[k] + c[k] for k in R.HEAD}
        for a in range(A):
            eps[a] += ep[a]
        # last_stats: this rollout's record, means over max(episodes, 1)
        assert ls['episodes'] == n and ls['ep_length'] == c['sum_len'] / max(n, 1)
        assert ls['win_rate'] == c['wins0'] / max(n, 1) and len(ls['ep_return']) == A
    got = state4['total'].cpu().numpy()
    print('total', got.tolist())
    assert total['episodes'] > 0, 'no episode finished: the short-episode config did not shorten them'
    assert got[:6].tolist() == [float(total[k]) for k in R.HEAD]
    assert total['wins0'] + total['wins1'] + total['draws'] == total['episodes']
    q = R.check_sums(got, total, eps)
    print(f'sums {q:.3f} of the bound ({total["episodes"]} episodes)')
    assert q <= 1.0
    last = state4['last'].cpu().numpy()
    assert last[:6].tolist() == [float(c[k]) for k in R.HEAD] and R.check_sums(last, c, ep) <= 1.0
    assert state4['ret_carry'].cpu().tolist() == G and state4['len_carry'].cpu().tolist() == ln
    s = tr.episode_summary()
    assert s['episodes'] == total['episodes'] and s['wins'] == [total['wins0'], total['wins1']]
    assert s['mean_length'] == total['sum_len'] / total['episodes'] and len(s['return']) == A
    # every agent's columns, under self-play too: the opponent's agents have returns of their own
    assert any(x != 0.0 for x in eps[2] + eps[3])


def test_flag_on_and_off_train_the_same_parameters(trained):
    selfplay, _, records, _, _, _, params_on, _ = trained
    env = _env()
    off = _trainer(env, selfplay)
    for _ in range(ITERS):
        off.iteration()
    assert off.ep_stats is None and not set(EP_KEYS) & set(off.last_stats) and 'ep_stats' not in off.state_dict()
    assert torch.equal(_bits(_params(off)), _bits(params_on))  # the feature only reads
    assert np.array_equal(off.buf.rewards.reshape(T, -1).cpu().numpy(), records[-1][0])
    env.close()


def test_checkpoint_resumes_the_totals_of_the_uninterrupted_run(trained):
    selfplay, _, _, _, state2, state4, params_on, path = trained
    sd = torch.load(path, map_location='cpu', weights_only=True)
    assert set(sd['ep_stats']) == {'ret_carry', 'len_carry', 'last', 'total', 'n_agents', 'side_mask'}
    env = _env(first_seed=300)  # (the checkpoint brings the env state)
    tr2 = _trainer(env, selfplay, episode_stats=True)
    tr2.load(path)
    for k, v in _state(tr2).items():
        assert torch.equal(_bits(v), _bits(state2[k])), k
    for _ in range(ITERS - 2):
        tr2.iteration()
    for k, v in _state(tr2).items():
        assert torch.equal(_bits(v), _bits(state4[k])), k
    assert torch.equal(_bits(_params(tr2)), _bits(params_on))
    assert float(state4['total'][0]) > float(state2['total'][0]) > 0
    env.close()
