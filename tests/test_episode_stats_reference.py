"""Episode statistics, host side (no GPU): the torch restatement of
mas_episode_stats (masurvival.ppo.episode_stats_reference) against the plain
Python loop of tests/ep_ref.py and a hand-written known answer, chaining
through the carries, EpisodeStats on the CPU, two gloo ranks, and the trainer on
the CPU stand-in env of tests/test_ppo.py (restated here): the new last_stats
keys, checkpoints, the flag off."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ep_ref as R
from masurvival.ppo import (EPISODE_RECORD_HEAD, EpisodeStats, PPOConfig, PPOTrainer, PolicyMLP,
                            episode_stats_reference, gae_reference_into)

F32 = np.float32
T_H = 6  # the trainers' horizon
EP_KEYS = {'episodes', 'ep_length', 'ep_return', 'win_rate'}


class StandInEnv:
    """Deterministic CPU env with VecMaSurvival's step/reset surface (the test
    double of tests/test_ppo.py)."""

    def __init__(self, n_envs=8, n_agents=4, obs_dim=12, seed=0):
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


def _data(T=17, E=43, A=3, p_done=0.1, seed=0, half=False):
    rng = np.random.default_rng(seed)
    if half:
        r = (rng.integers(-2, 3, size=(T, E * A)) * 0.5).astype(F32)
        G = rng.integers(-6, 7, size=E * A) * 0.5
    else:
        r = rng.standard_normal((T, E * A)).astype(F32)
        G = 3.0 * rng.standard_normal(E * A)
    d = (rng.random((T, E)) < p_done).astype(np.uint8)
    d[d != 0] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=int((d != 0).sum()))
    return r, d, G.astype(np.float64), rng.integers(0, 40, size=E).astype(np.int32)


def _reference(r, d, A, G, ln, mask):
    tg, tl = torch.from_numpy(G), torch.from_numpy(ln)
    keep = (tg.clone(), tl.clone())
    g, n, rec = episode_stats_reference(torch.from_numpy(r), torch.from_numpy(d), A, tg, tl, mask)
    assert torch.equal(tg, keep[0]) and torch.equal(tl, keep[1]), 'a carry going in was written'
    assert g.dtype == torch.float64 and n.dtype == torch.int32 and rec.dtype == torch.float64
    assert g.shape == (len(G),) and n.shape == (len(ln),) and rec.shape == (6 + 2 * A,)
    return g.numpy(), n.numpy(), rec.numpy()


def test_known_answer_written_down_by_hand():
    """2 envs x 2 agents, side 0 = agent 0, two calls of T = 5.  (a0, a1) per step:
    env 0: (1, .5) (.5, 1)D | (1, 0) (1, 0) (0, -.5) || (.5, .5)D | zeros
           episode 1: G = (1.5, 1.5), length 2, a draw; episode 2 straddles the
           calls: G = (2.5, 0), length 4, side 0 wins
    env 1: (0, 1) (0, 1) (.5, 1) (-1, 0)D | (2, 0)D || (0, .25) x 5
           G = (-.5, 3), length 4, side 1 wins; G = (2, 0), length 1, side 0 wins"""
    r1 = np.array([[1, .5, 0, 1], [.5, 1, 0, 1], [1, 0, .5, 1], [1, 0, -1, 0], [0, -.5, 2, 0]], dtype=F32)
    d1 = np.array([[0, 0], [1, 0], [0, 0], [0, 7], [0, 255]], dtype=np.uint8)
    r2 = np.array([[.5, .5, 0, .25]] + [[0, 0, 0, .25]] * 4, dtype=F32)
    d2 = np.array([[1, 0]] + [[0, 0]] * 4, dtype=np.uint8)
    want1 = [3, 7, 21, 1, 1, 1, 3.0, 4.5, 6.5, 11.25]
    want2 = [1, 4, 16, 1, 0, 0, 2.5, 0.0, 6.25, 0.0]
    G, ln = np.zeros(4), np.zeros(2, dtype=np.int32)
    g1, n1, rec1 = _reference(r1, d1, 2, G, ln, 0b01)
    assert rec1.tolist() == want1 and g1.tolist() == [2.0, -0.5, 0.0, 0.0] and n1.tolist() == [3, 0]
    g2, n2, rec2 = _reference(r2, d2, 2, g1, n1, 0b01)
    assert rec2.tolist() == want2 and g2.tolist() == [0.0, 0.0, 0.0, 1.25] and n2.tolist() == [4, 5]
    # the plain loop says the same
    pg, pn, c, ep = R.walk(r1, d1, 2, G, ln, 0b01)
    assert R.record(c, ep) == want1 and pg == g1.tolist() and pn == n1.tolist()
    pg, pn, c, ep = R.walk(r2, d2, 2, pg, pn, 0b01)
    assert R.record(c, ep) == want2 and pg == g2.tolist() and pn == n2.tolist()
    # the other side's view swaps the wins; no sides: no wins, the rest unchanged
    assert _reference(r1, d1, 2, G, ln, 0b10)[2].tolist() == want1[:3] + [1, 1, 1] + want1[6:]
    for mask in (0, 0b11):
        assert _reference(r1, d1, 2, G, ln, mask)[2].tolist() == want1[:3] + [0, 0, 0] + want1[6:]
    assert EPISODE_RECORD_HEAD == R.HEAD
    with pytest.raises(ValueError):
        episode_stats_reference(torch.from_numpy(r1), torch.from_numpy(d1), 2, torch.zeros(4, dtype=torch.float64),
                                torch.zeros(2, dtype=torch.int32), 0b100)


@pytest.mark.parametrize('E,A,mask,half', [(43, 3, 0b101, False), (43, 3, 0b101, True), (9, 4, 0b0011, True),
                                           (9, 4, 0b0101, False), (5, 1, 0, False), (7, 8, 0x0F, True),
                                           (7, 5, 0b11111, False), (6, 9, 0b1, False)])
def test_restatement_against_the_plain_loop(E, A, mask, half):
    r, d, G, ln = _data(E=E, A=A, p_done=0.15, seed=E + A, half=half)
    g, n, rec = _reference(r, d, A, G, ln, mask)
    pg, pn, c, ep = R.walk(r, d, A, G, ln, mask)
    assert c['episodes'] > 0
    assert np.array_equal(g.view(np.int64), np.array(pg).view(np.int64)), 'ret_carry: one order, bit for bit'
    assert n.tolist() == pn
    assert rec[:6].tolist() == [float(c[k]) for k in R.HEAD]
    if half:
        assert rec.tolist() == R.record(c, ep)  # every sum is exact
    q = R.check_sums(rec, c, ep)
    print(f'worst |d| / bound: {q:.3f}')
    assert q <= 1.0
    if mask in (0, (1 << A) - 1):
        assert rec[3:6].tolist() == [0, 0, 0]
    else:
        assert rec[3] + rec[4] + rec[5] == rec[0]


def test_a_nan_return_is_none_of_win_loss_or_draw():
    r = np.array([[1, float('nan')], [1, 1]], dtype=F32)
    d = np.array([[1], [1]], dtype=np.uint8)
    _, _, rec = _reference(r, d, 2, np.zeros(2), np.zeros(1, dtype=np.int32), 0b01)
    assert rec[:6].tolist() == [2, 2, 2, 0, 0, 1] and rec[6] == 2.0 and math.isnan(rec[7])
    assert R.walk(r, d, 2, [0, 0], [0], 0b01)[2] == dict(zip(R.HEAD, (2, 2, 2, 0, 0, 1)))


def test_two_rollouts_chain_through_the_carries():
    """Rows [0, 9) then [9, 26) from the first call's carries: the carries of
    one 26-row call bit for bit, integer entries that add up exactly."""
    A, mask = 3, 0b011
    r, d, G, ln = _data(T=26, E=86, A=A, p_done=0.05, seed=5)
    g_all, n_all, rec_all = _reference(r, d, A, G, ln, mask)
    g_a, n_a, rec_a = _reference(r[:9].copy(), d[:9].copy(), A, G, ln, mask)
    g_b, n_b, rec_b = _reference(r[9:].copy(), d[9:].copy(), A, g_a, n_a, mask)
    assert np.array_equal(g_b.view(np.int64), g_all.view(np.int64)) and np.array_equal(n_b, n_all)
    assert (rec_a[:6] + rec_b[:6]).tolist() == rec_all[:6].tolist() and rec_all[0] > 0
    _, _, c, ep = R.walk(r, d, A, G, ln, mask)
    assert R.check_sums(rec_a + rec_b, c, ep) <= 2.0  # two partial sums and the addition here


def test_episode_stats_on_the_cpu_totals_summary_and_state():
    E, A, mask = 7, 3, 0b001
    es = EpisodeStats(E, A, 'cpu', side_mask=mask)
    assert es.ret_carry.dtype == torch.float64 and es.ret_carry.shape == (E * A,) and not es.ret_carry.any()
    assert es.len_carry.dtype == torch.int32 and es.len_carry.shape == (E,)
    assert es.last.shape == es.total.shape == (6 + 2 * A,) and es.total.dtype == torch.float64
    for which in ('last', 'total'):
        s = es.summary(which)  # nothing finished: zeros, no NaN
        assert s == {'episodes': 0, 'mean_length': 0.0, 'std_length': 0.0, 'return': [0.0] * A,
                     'return_std': [0.0] * A, 'wins': [0, 0], 'draws': 0, 'win_rate': 0.0}
    G, ln = np.zeros(E * A), np.zeros(E, dtype=np.int32)
    lasts, eps = [], [[] for _ in range(A)]
    counts = dict.fromkeys(R.HEAD, 0)
    for k, T in enumerate((5, 1, 12)):
        r, d, _, _ = _data(T=T, E=E, A=A, p_done=0.3, seed=10 + k, half=True)
        tr, td = torch.from_numpy(r).view(T, E, A), torch.from_numpy(d)
        keep = tr.clone()
        es.update(tr, td)
        assert torch.equal(tr, keep)
        G, ln, c, ep = R.walk(r, d, A, G, ln, mask)
        assert es.last.tolist() == R.record(c, ep)
        assert es.ret_carry.tolist() == G and es.len_carry.tolist() == ln
        lasts.append(es.last.clone())
        for a in range(A):
            eps[a] += ep[a]
        counts = {k_: counts[k_] + c[k_] for k_ in R.HEAD}
    assert torch.equal(es.total, lasts[0] + lasts[1] + lasts[2]) and es.total.tolist() == R.record(counts, eps)
    s, n = es.summary('total'), counts['episodes']
    assert n > 3 and s['episodes'] == n and s['wins'] == [counts['wins0'], counts['wins1']]
    assert s['draws'] == counts['draws'] and s['win_rate'] == counts['wins0'] / n
    assert s['mean_length'] == counts['sum_len'] / n
    assert abs(s['std_length'] - math.sqrt(counts['sum_len2'] / n - (counts['sum_len'] / n) ** 2)) < 1e-12
    for a in range(A):
        assert abs(s['return'][a] - np.mean(eps[a])) < 1e-12 and abs(s['return_std'][a] - np.std(eps[a])) < 1e-9
    assert es.summary() == es.summary('last') and es.summary('last')['episodes'] == int(lasts[2][0])
    assert all(type(v) in (int, float, list) for v in s.values())
    with pytest.raises(ValueError):
        es.summary('all')
    # the state round-trips; another shape or side is refused
    sd = es.state_dict()
    assert set(sd) == {'ret_carry', 'len_carry', 'last', 'total', 'n_agents', 'side_mask'}
    back = EpisodeStats.from_state_dict(sd, 'cpu')
    for name in ('ret_carry', 'len_carry', 'last', 'total'):
        assert torch.equal(getattr(back, name), getattr(es, name)), name
    assert (back.n_envs, back.n_agents, back.side_mask) == (E, A, mask)
    for other in (EpisodeStats(E + 1, A, 'cpu', mask), EpisodeStats(E, A + 1, 'cpu', mask),
                  EpisodeStats(E, A, 'cpu', 0b010)):
        with pytest.raises(ValueError):
            other.load_state_dict(sd)
    with pytest.raises(ValueError):
        es.update(torch.zeros((4, E + 1, A)), torch.zeros((4, E + 1), dtype=torch.uint8))
    with pytest.raises(ValueError):
        EpisodeStats(E, A, 'cpu', side_mask=0b1000)


def _trainer(env, **kw):
    cfg = PPOConfig(horizon=T_H, hidden=32, minibatches=2, autocast_bf16=False, **kw)
    tr = PPOTrainer(env, cfg, seed=3)
    tr.gae_impl = gae_reference_into
    return tr


def _recorded_iteration(tr):
    """One iteration; (rewards, dones) of its rollout as numpy copies."""
    tr.iteration()
    b = tr.buf
    return b.rewards.reshape(T_H, -1).numpy().copy(), b.dones.numpy().copy()


def test_cpu_trainer_reports_the_episodes_of_its_rollouts():
    env = StandInEnv()
    tr = _trainer(env, episode_stats=True)
    A, E = env.n_agents, env.n_envs
    assert tr.ep_stats.side_mask == 0b0011 and tr.ep_stats.n_envs == E and tr.ep_stats.n_agents == A
    G, ln = [0.0] * (E * A), [0] * E
    total = dict.fromkeys(R.HEAD, 0)
    for it in range(3):
        r, d = _recorded_iteration(tr)
        G, ln, c, ep = R.walk(r, d, A, G, ln, 0b0011)
        assert tr.ep_stats.last.tolist() == R.record(c, ep)  # the stand-in's rewards are half-integers: exact
        assert tr.ep_stats.ret_carry.tolist() == G and tr.ep_stats.len_carry.tolist() == ln
        total = {k: total[k] + c[k] for k in R.HEAD}
        ls, n = tr.last_stats, c['episodes']
        assert n > 0 and EP_KEYS <= set(ls)
        assert all(isinstance(ls[k], torch.Tensor) and ls[k].dtype == torch.float64 for k in EP_KEYS)
        assert float(ls['episodes']) == n and float(ls['ep_length']) == c['sum_len'] / n
        assert ls['ep_return'].shape == (A,) and ls['ep_return'].tolist() == [math.fsum(g) / n for g in ep]
        assert float(ls['win_rate']) == c['wins0'] / n
    assert tr.ep_stats.total[:6].tolist() == [float(total[k]) for k in R.HEAD]
    s = tr.episode_summary()
    assert s == tr.ep_stats.summary('total') and s['episodes'] == total['episodes']
    assert tr.episode_summary('last')['episodes'] == c['episodes']
    assert torch.isfinite(tr.last_stats['loss'])
    # one agent has no sides; an opponent makes the learner's agents side 0, over every agent's columns
    assert _trainer(StandInEnv(n_agents=1), episode_stats=True).ep_stats.side_mask == 0
    env2 = StandInEnv()
    sp = PPOTrainer(env2, PPOConfig(horizon=T_H, hidden=32, minibatches=2, autocast_bf16=False, episode_stats=True),
                    seed=3, opponent=PolicyMLP(env2.obs_dim, 32), learner_agents=[0, 2])
    sp.gae_impl = gae_reference_into
    assert sp.ep_stats.side_mask == 0b0101 and sp.ep_stats.n_agents == 4
    r, d = _recorded_iteration(sp)
    _, _, c, ep = R.walk(r, d, 4, [0.0] * 32, [0] * 8, 0b0101)
    assert sp.ep_stats.last.tolist() == R.record(c, ep) and sp.last_stats['ep_return'].shape == (4,)


def test_no_episode_in_a_rollout_gives_zeros_and_no_nan():
    env = StandInEnv()
    tr = _trainer(env, episode_stats=True)
    env.step = lambda actions, out=None, f=env.step: (f(actions, out), out[2].zero_())[0]  # nothing ever ends
    tr.iteration()
    ls = tr.last_stats
    assert float(ls['episodes']) == 0 and float(ls['ep_length']) == 0 and float(ls['win_rate']) == 0
    assert ls['ep_return'].tolist() == [0.0] * 4 and tr.ep_stats.len_carry.tolist() == [T_H] * 8
    assert tr.episode_summary()['episodes'] == 0


def test_checkpoint_resume_continues_the_totals_of_an_uninterrupted_run(tmp_path):
    tr = _trainer(StandInEnv(), episode_stats=True)
    tr.iteration()
    path = str(tmp_path / 'ckpt.pt')
    tr.save(path)
    sd = torch.load(path, weights_only=True)
    assert set(sd['ep_stats']) == {'ret_carry', 'len_carry', 'last', 'total', 'n_agents', 'side_mask'}
    assert sd['ep_stats']['ret_carry'].dtype == torch.float64 and sd['ep_stats']['len_carry'].dtype == torch.int32
    tr.iteration()
    tr2 = _trainer(StandInEnv(seed=99), episode_stats=True)
    tr2.load(path)
    assert torch.equal(tr2.ep_stats.total, sd['ep_stats']['total'])
    tr2.iteration()
    for name in ('total', 'last', 'ret_carry', 'len_carry'):
        assert torch.equal(getattr(tr.ep_stats, name), getattr(tr2.ep_stats, name)), name
    assert tr.episode_summary() == tr2.episode_summary() and tr.episode_summary()['episodes'] > 0
    for a, b in zip(tr.policy.parameters(), tr2.policy.parameters()):
        assert torch.equal(a, b)
    # the flag off: the checkpoint's statistics are restored, kept and saved again, not updated
    tr3 = _trainer(StandInEnv(seed=5))
    assert tr3.ep_stats is None and 'ep_stats' not in tr3.state_dict()
    with pytest.raises(ValueError):
        tr3.episode_summary()
    tr3.load(path)
    assert torch.equal(tr3.ep_stats.total, sd['ep_stats']['total'])
    tr3.iteration()
    assert torch.equal(tr3.ep_stats.total, sd['ep_stats']['total']) and 'ep_stats' in tr3.state_dict()
    assert not EP_KEYS & set(tr3.last_stats)
    # another env count is refused
    with pytest.raises(ValueError):
        _trainer(StandInEnv(n_envs=4), episode_stats=True).load_state_dict(sd)
    # a checkpoint without the key leaves a flagged trainer's fresh state alone
    old = _trainer(StandInEnv())
    old.iteration()
    old_path = str(tmp_path / 'old.pt')
    old.save(old_path)
    tr4 = _trainer(StandInEnv(seed=1), episode_stats=True)
    tr4.load(old_path)
    assert not tr4.ep_stats.total.any() and not tr4.ep_stats.ret_carry.any()
    tr4.iteration()
    assert float(tr4.ep_stats.total[0]) > 0


def test_flag_off_is_the_trainer_without_the_flag():
    a = PPOTrainer(StandInEnv(), PPOConfig(horizon=T_H, hidden=32, minibatches=2, autocast_bf16=False), seed=3)
    a.gae_impl = gae_reference_into
    b = _trainer(StandInEnv(), episode_stats=False)
    on = _trainer(StandInEnv(), episode_stats=True)
    for tr in (a, b, on):
        tr.iteration()
    assert set(a.last_stats) == set(b.last_stats) == {'loss', 'pg', 'v'}  # exactly today's keys
    assert set(on.last_stats) == {'loss', 'pg', 'v'} | EP_KEYS
    assert b.ep_stats is None and PPOConfig().episode_stats is False
    for tr in (b, on):  # the feature only reads
        for p, q in zip(a.policy.parameters(), tr.policy.parameters()):
            assert torch.equal(p, q)
        assert torch.equal(a.buf.adv, tr.buf.adv) and torch.equal(a.buf.ret, tr.buf.ret)


def _rank_main(rank, world, init_file, out_dir):
    dist.init_process_group('gloo', init_method=f'file://{init_file}', rank=rank, world_size=world)
    torch.set_num_threads(1)
    tr = _trainer(StandInEnv(seed=100 + rank), episode_stats=True)
    # different episodes per rank: rank 1's env clock runs three steps ahead
    tr.env.t = 3 * rank
    rec = [_recorded_iteration(tr) for _ in range(2)]
    torch.save({'last': tr.ep_stats.last, 'total': tr.ep_stats.total, 'ret_carry': tr.ep_stats.ret_carry,
                'len_carry': tr.ep_stats.len_carry,
                'rewards': torch.from_numpy(np.stack([r for r, _ in rec])),
                'dones': torch.from_numpy(np.stack([d for _, d in rec]))}, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_gloo_records_are_summed_and_the_carries_stay_per_rank(tmp_path):
    ctx = mp.get_context('spawn')
    init_file = str(tmp_path / 'rdzv')
    ps = [ctx.Process(target=_rank_main, args=(r, 2, init_file, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(150)
        assert p.exitcode == 0
    res = [torch.load(str(tmp_path / f'rank{r}.pt'), weights_only=True) for r in range(2)]
    assert torch.equal(res[0]['last'], res[1]['last']) and torch.equal(res[0]['total'], res[1]['total'])
    assert not torch.equal(res[0]['len_carry'], res[1]['len_carry'])
    assert not torch.equal(res[0]['ret_carry'], res[1]['ret_carry'])
    # each rank's own records, by the plain loop over what it saw
    own_last, own_total = np.zeros(14), np.zeros(14)
    for k in range(2):
        G, ln = [0.0] * 32, [0] * 8
        for it in range(2):
            G, ln, c, ep = R.walk(res[k]['rewards'][it].numpy(), res[k]['dones'][it].numpy(), 4, G, ln, 0b0011)
            own_total += np.array(R.record(c, ep))
        own_last += np.array(R.record(c, ep))
        assert res[k]['ret_carry'].tolist() == G and res[k]['len_carry'].tolist() == ln
    assert res[0]['last'].tolist() == own_last.tolist() and res[0]['total'].tolist() == own_total.tolist()
    assert own_last[0] > 0
