"""Running observation normalisation, host side (no GPU): the fold
W1 ((x - mu) * s) + b1 = (W1 diag(s)) x + (b1 - W1 (mu * s)) and the gradient
unfold in fp64, the torch restatement of the moments and of Chan's merge, and
the trainer on the CPU stand-in env of tests/test_ppo.py (restated here):
what it merges and when, checkpoints, match.load_policy, two gloo ranks."""
import copy
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from masurvival.match import load_policy
from masurvival.ppo import (ObsNorm, PolicyMLP, PPOConfig, PPOTrainer, gae_reference_into, merge_reference,
                            obs_moments_reference, unfold_dw1)


class StandInEnv:
    """Deterministic CPU env with VecMaSurvival's step/reset surface (the test
    double of tests/test_ppo.py), its columns at different offsets and scales."""

    def __init__(self, n_envs=8, n_agents=4, obs_dim=12, seed=0):
        self.n_envs, self.n_agents, self.obs_dim = n_envs, n_agents, obs_dim
        self.device = torch.device('cpu')
        self.g = torch.Generator().manual_seed(seed)
        self.t = 0
        self.scale = torch.linspace(0.1, 20.0, obs_dim)
        self.offset = torch.linspace(-50.0, 100.0, obs_dim)

    def _draw(self, shape):
        return torch.randn(shape, generator=self.g) * self.scale + self.offset

    def reset(self):
        return self._draw((self.n_envs, self.n_agents, self.obs_dim))

    def step(self, actions, out=None):
        self.t += 1
        o, r, d = out
        o.copy_(self._draw(o.shape))
        r.copy_((actions[..., 0].float() - 1.0) * 0.5 + (actions[..., 3].float()))
        d.copy_(((torch.arange(self.n_envs) + self.t) % 5 == 0).to(torch.uint8))
        return o, r, d, {}

    def get_state(self):
        return torch.cat([self.g.get_state(), torch.tensor([self.t], dtype=torch.int64).view(torch.uint8)])

    def set_state(self, buf):
        self.g.set_state(buf[:-8].clone())
        self.t = int(buf[-8:].clone().view(torch.int64)[0])


def _normed_and_folded(D=13, hidden=32, seed=0):
    """(policy with a normaliser, the same policy with the normaliser folded
    into layer 1 on the host), both fp64."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    p = PolicyMLP(D, hidden).double()
    mean = (torch.rand((D,), generator=g, dtype=torch.float64) * 2 - 1) * 100
    s = 0.05 + torch.rand((D,), generator=g, dtype=torch.float64) * 9.95
    folded = copy.deepcopy(p)
    with torch.no_grad():
        w1f = p.body[0].weight * s
        folded.body[0].weight.copy_(w1f)
        folded.body[0].bias.copy_(p.body[0].bias - w1f @ mean)
    p.set_obs_norm(mean, s)
    return p, folded, mean, s, g


def test_normalised_policy_equals_the_folded_one_on_raw_rows():
    p, folded, mean, s, g = _normed_and_folded()
    assert folded.obs_mean is None
    x = torch.randn((257, 13), generator=g, dtype=torch.float64) / s + mean  # normalised inputs are O(1)
    torch.testing.assert_close(p.forward_raw(x), folded.forward_raw(x), rtol=1e-12, atol=1e-12)
    la, va = p(x)
    lb, vb = folded(x)
    torch.testing.assert_close(la, lb, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(va, vb, rtol=1e-12, atol=1e-12)


def test_policy_state_dict_keys_do_not_change_and_copies_keep_the_normaliser():
    p, _, mean, s, _ = _normed_and_folded()
    plain = PolicyMLP(13, 32)
    assert list(p.state_dict().keys()) == list(plain.state_dict().keys())
    plain.load_state_dict({k: v.float() for k, v in p.state_dict().items()})  # an old checkpoint's keys load
    q = copy.deepcopy(p)
    assert torch.equal(q.obs_mean, mean) and torch.equal(q.obs_inv_std, s) and q.obs_mean is not p.obs_mean
    assert p.float().obs_mean.dtype == torch.float32
    with pytest.raises(ValueError):
        p.set_obs_norm(mean, None)
    with pytest.raises(ValueError):
        p.set_obs_norm(mean[:-1], s[:-1])
    p.set_obs_norm(None, None)
    assert p.obs_mean is None


def test_unfold_dw1_gives_autograd_dw1_of_the_normalised_form():
    p, folded, mean, s, g = _normed_and_folded(seed=1)
    x = torch.randn((300, 13), generator=g, dtype=torch.float64) / s + mean
    w = torch.randn((300, 16), generator=g, dtype=torch.float64)
    (p.forward_raw(x) * w).sum().backward()
    (folded.forward_raw(x) * w).sum().backward()
    l1, f1 = p.body[0], folded.body[0]
    dw1 = unfold_dw1(f1.weight.grad, f1.bias.grad, mean, s)
    torch.testing.assert_close(dw1, l1.weight.grad, rtol=1e-9, atol=1e-9 * float(l1.weight.grad.abs().max()))
    torch.testing.assert_close(f1.bias.grad, l1.bias.grad, rtol=1e-12, atol=1e-12)
    for a, b in zip(list(p.parameters())[2:], list(folded.parameters())[2:]):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-10, atol=1e-12)


def _bf16_rows(rows, cols, g, offset_to=100.0):
    x = torch.randn((rows, cols), generator=g) * 3 + torch.linspace(-offset_to, offset_to, cols)
    return x.to(torch.bfloat16)


def _batch(x, n_cols):
    return torch.cat([torch.tensor([float(x.shape[0])], dtype=torch.float64),
                      obs_moments_reference(x, n_cols).reshape(-1)])


def test_merging_three_batches_equals_the_moments_of_their_concatenation():
    g = torch.Generator().manual_seed(2)
    D = 11
    xs = [_bf16_rows(n, D + 5, g) for n in (7, 1, 259)]
    state = torch.zeros((1 + 2 * D,), dtype=torch.float64)
    for x in xs:
        mean32, inv32 = merge_reference(state, _batch(x, D), 1e-2)
    allx = torch.cat(xs)[:, :D].double()
    n = allx.shape[0]
    mean = allx.mean(0)
    m2 = ((allx - mean) ** 2).sum(0)
    assert float(state[0]) == n
    torch.testing.assert_close(state[1:1 + D], mean, rtol=1e-12, atol=0)
    torch.testing.assert_close(state[1 + D:], m2, rtol=1e-12, atol=0)
    torch.testing.assert_close(mean32, mean.float(), rtol=2e-7, atol=1e-12)  # one fp32 ulp
    torch.testing.assert_close(inv32, (1.0 / torch.sqrt(m2 / n + 1e-2)).float(), rtol=2e-7, atol=0)
    assert float(inv32.max()) <= 10.0  # the variance floor: 1 / sqrt(eps)


def test_zero_row_batch_changes_nothing_and_an_empty_state_is_the_identity():
    D = 5
    state = torch.zeros((1 + 2 * D,), dtype=torch.float64)
    mean32, inv32 = merge_reference(state, torch.zeros_like(state), 1e-2)
    assert torch.equal(state, torch.zeros_like(state))
    assert torch.equal(mean32, torch.zeros(D)) and torch.equal(inv32, torch.ones(D))
    g = torch.Generator().manual_seed(3)
    x = _bf16_rows(33, D, g)
    a = merge_reference(state, _batch(x, D), 1e-2)
    before = state.clone()
    b = merge_reference(state, _batch(x[:0], D), 1e-2)
    assert torch.equal(state, before) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ObsNorm on the CPU is that restatement
    on = ObsNorm(D, 'cpu')
    assert torch.equal(on.mean, torch.zeros(D)) and torch.equal(on.inv_std, torch.ones(D))
    on.update(x)
    assert torch.equal(on.state, before) and torch.equal(on.mean, a[0]) and torch.equal(on.inv_std, a[1])
    on.update(x[:0])
    assert torch.equal(on.state, before) and torch.equal(on.inv_std, a[1])
    with pytest.raises(ValueError):
        on.update(x.float())
    back = ObsNorm.from_state_dict(on.state_dict(), 'cpu')
    assert torch.equal(back.state, on.state) and torch.equal(back.mean, on.mean)
    assert torch.equal(back.inv_std, on.inv_std)
    assert all(v.dtype == torch.float64 for k, v in on.state_dict().items() if k != 'eps')


def _trainer(env, **kw):
    cfg = PPOConfig(horizon=6, hidden=32, minibatches=2, autocast_bf16=False, **kw)
    tr = PPOTrainer(env, cfg, seed=3)
    tr.gae_impl = gae_reference_into
    return tr


def test_trainer_merges_block_0_then_each_iterations_blocks():
    env = StandInEnv()
    tr = _trainer(env, obs_norm=True)
    D, T = env.obs_dim, 6
    ref = torch.zeros((1 + 2 * D,), dtype=torch.float64)
    rows = lambda o: o.reshape(-1, D).to(torch.bfloat16)  # noqa: E731
    want = merge_reference(ref, _batch(rows(tr.buf.obs[0]), D), 1e-2)
    assert torch.equal(tr.obs_norm.state, ref) and float(ref[0]) == 32
    assert tr.policy.obs_mean is tr.obs_norm.mean and torch.equal(tr.policy.obs_inv_std, want[1])
    for it in range(2):
        first = tr.buf.obs[0].clone()  # block 0 is overwritten by the next rollout's first rows
        tr.iteration()
        blocks = torch.cat([first.unsqueeze(0), tr.buf.obs[1:T]])
        want = merge_reference(ref, _batch(rows(blocks), D), 1e-2)
        assert torch.equal(tr.obs_norm.state, ref), it
        assert torch.equal(tr.obs_norm.mean, want[0]) and torch.equal(tr.obs_norm.inv_std, want[1])
    assert float(ref[0]) == 32 * (1 + 2 * T)
    assert torch.isfinite(tr.last_stats['loss'])
    # the columns arrive at their scales: the normaliser has learnt them
    torch.testing.assert_close(tr.obs_norm.mean, env.offset, rtol=0.2, atol=1.0)


def test_checkpoint_round_trip_and_load_policy(tmp_path):
    env = StandInEnv()
    tr = _trainer(env, obs_norm=True)
    tr.iteration()
    path = str(tmp_path / 'ckpt.pt')
    tr.save(path)
    sd = torch.load(path, weights_only=True)
    assert set(sd['obs_norm']) == {'count', 'mean', 'm2', 'eps'}
    x = StandInEnv(seed=7).reset()  # (not env's: its generator belongs to the run that goes on below)
    # load_policy: the same function of raw rows as the trainer's policy
    pol = load_policy(path)
    assert torch.equal(pol.forward_raw(x), tr.policy.forward_raw(x))
    assert list(pol.state_dict().keys()) == list(tr.policy.state_dict().keys())
    # a fresh trainer resumes the same normaliser and continues the same trajectory
    tr.iteration()
    tr2 = _trainer(StandInEnv(seed=99), obs_norm=True)
    tr2.load(path)
    tr2.iteration()
    assert torch.equal(tr.obs_norm.state, tr2.obs_norm.state)
    for a, b in zip(tr.policy.parameters(), tr2.policy.parameters()):
        assert torch.equal(a, b)
    # the flag off: the checkpoint's normaliser is restored and applied, not updated
    tr3 = _trainer(StandInEnv(seed=5))
    assert tr3.obs_norm is None and 'obs_norm' not in tr3.state_dict()
    tr3.load(path)
    assert torch.equal(tr3.obs_norm.state[1:1 + env.obs_dim], sd['obs_norm']['mean'])
    assert torch.equal(tr3.policy.forward_raw(x), pol.forward_raw(x))
    frozen = tr3.obs_norm.state.clone()
    tr3.iteration()
    assert torch.equal(tr3.obs_norm.state, frozen)
    assert 'obs_norm' in tr3.state_dict()


def test_checkpoint_without_the_key_loads_and_the_flag_off_writes_none(tmp_path):
    tr = _trainer(StandInEnv())
    tr.iteration()
    sd = tr.state_dict()
    assert 'obs_norm' not in sd
    path = str(tmp_path / 'old.pt')
    tr.save(path)
    assert load_policy(path).obs_mean is None
    # into a trainer that normalises: its own statistics stay
    tr2 = _trainer(StandInEnv(seed=1), obs_norm=True)
    before = tr2.obs_norm.state.clone()
    tr2.load(path)
    assert torch.equal(tr2.obs_norm.state, before)
    tr2.iteration()
    assert torch.isfinite(tr2.last_stats['loss'])


def test_flag_off_is_the_trainer_without_the_flag():
    a = PPOTrainer(StandInEnv(), PPOConfig(horizon=6, hidden=32, minibatches=2, autocast_bf16=False), seed=3)
    b = _trainer(StandInEnv(), obs_norm=False)
    a.gae_impl = gae_reference_into
    a.iteration()
    b.iteration()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert b.obs_norm is None and b.policy.obs_mean is None


def test_self_play_merges_the_learners_rows_and_sync_copies_the_normaliser():
    env = StandInEnv()
    opp = PolicyMLP(env.obs_dim, 32)
    tr = PPOTrainer(env, PPOConfig(horizon=6, hidden=32, minibatches=2, autocast_bf16=False, obs_norm=True,
                                   opponent_sync_every=1), seed=3, opponent=opp, learner_agents=[0, 2])
    tr.gae_impl = gae_reference_into
    D = env.obs_dim
    assert float(tr.obs_norm.count) == env.n_envs * 2
    ref = torch.zeros((1 + 2 * D,), dtype=torch.float64)
    merge_reference(ref, _batch(tr.buf.obs[0][:, [0, 2]].reshape(-1, D).to(torch.bfloat16), D), 1e-2)
    assert torch.equal(tr.obs_norm.state, ref)
    assert tr.opponent.obs_mean is None
    tr.iteration()
    assert float(tr.obs_norm.count) == env.n_envs * 2 * 7
    assert torch.equal(tr.opponent.obs_mean, tr.policy.obs_mean) and tr.opponent.obs_mean is not tr.policy.obs_mean
    sd = tr.state_dict()
    assert torch.equal(sd['opponent_obs_norm']['inv_std'], tr.policy.obs_inv_std)


def _rank_main(rank, world, init_file, out_dir):
    dist.init_process_group('gloo', init_method=f'file://{init_file}', rank=rank, world_size=world)
    torch.set_num_threads(1)
    env = StandInEnv(seed=100 + rank)  # different data per rank
    tr = _trainer(env, obs_norm=True)
    first = float(tr.obs_norm.count)
    tr.iteration()
    tr.iteration()
    flat = torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()])
    torch.save({'flat': flat, 'state': tr.obs_norm.state, 'mean': tr.obs_norm.mean, 'inv_std': tr.obs_norm.inv_std,
                'first': first, 'obs0': tr.buf.obs[0]}, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_gloo_normaliser_is_identical_on_both_ranks(tmp_path):
    ctx = mp.get_context('spawn')
    init_file = str(tmp_path / 'rdzv')
    ps = [ctx.Process(target=_rank_main, args=(r, 2, init_file, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(150)
        assert p.exitcode == 0
    res = [torch.load(str(tmp_path / f'rank{r}.pt'), weights_only=True) for r in range(2)]
    assert not torch.equal(res[0]['obs0'], res[1]['obs0'])  # the ranks saw different rows
    for k in ('state', 'mean', 'inv_std', 'flat'):
        assert torch.equal(res[0][k], res[1][k]), k
    # the counts are global: both ranks' reset rows, then both ranks' rollouts
    assert res[0]['first'] == 2 * 32 and float(res[0]['state'][0]) == 2 * 32 * (1 + 2 * 6)
