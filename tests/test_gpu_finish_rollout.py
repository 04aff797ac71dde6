"""PPOTrainer.finish_rollout -- the seam between rollout and update -- on real
rollouts of 2v2 x 256 envs at horizon 16, every expectation read from the
buffers the rollout filled and worked out in float64 (tests/gae_ref.py):
`ret` within the GAE bound, `adv` within the composed bound (GAE, the
normalisation's sensitivity to the statistics, its own roundings), the
statistics triple, the masked statistics with the count clamped to 1, the
minibatch row weights, the count under collectives, the bootstrap row
values[horizon] as a fresh act call of the matching form, and bit-identical
results from equal seeds.

Trainer forms: plain with the env's bf16 rows (x_obs) and with fp32 obs,
mask_dead, and self-play on learner_agents [0, 1] with and without mask_dead
(GAE then runs on the learner's dense rows with n_agents = 2).  The masked
cases overwrite buf.active after the rollout with synthetic 0 / 1 patterns, so
no rollout has to last until an agent dies."""
import functools
import json
import math
import os

import numpy as np
import pytest

import gae_ref as G

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival.ppo import PolicyMLP, PPOConfig, PPOTrainer  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'configs', '2v2.json')) as _f:
    CFG_2V2 = json.load(_f)
N, T, MB = 256, 16, 2
LA = [0, 1]
F32 = np.float32
U = G.U
FORMS = {
    'plain_x': (dict(), False),
    'plain_obs': (dict(x_obs=False), False),
    'mask': (dict(mask_dead=True), False),
    'selfplay': (dict(), True),
    'selfplay_mask': (dict(mask_dead=True), True),
}
MASKED = [f for f, (kw, _) in FORMS.items() if kw.get('mask_dead')]
PATTERNS = ('mixed', 'chunk_zero', 'all_zero')
WORST = {}


def _make(form, **more):
    kw, selfplay = FORMS[form]
    env = VecMaSurvival(CFG_2V2, n_envs=N, seeds=range(N), auto_reset=True)
    extra = {}
    if selfplay:
        torch.manual_seed(77)
        extra = dict(opponent=PolicyMLP(env.obs_dim, 256), learner_agents=LA)
    tr = PPOTrainer(env, PPOConfig(horizon=T, minibatches=MB, **kw, **more), seed=0, **extra)
    assert tr.fused is not None and tr.x_obs == (form != 'plain_obs')
    assert (tr.buf.learner is not None) == selfplay and (tr.buf.active is not None) == bool(kw.get('mask_dead'))
    for t in range(T):
        tr.rollout_step(t)
    tr.buf.values[T].fill_(float('nan'))   # finish_rollout has to write the bootstrap row
    torch.cuda.synchronize()
    return tr


@functools.lru_cache(maxsize=None)
def _rolled(form):
    """The trainer of the form after T rollout steps (finish_rollout can be
    called on it any number of times), with what it must leave alone."""
    tr = _make(form)
    b = tr.buf
    return tr, dict(steps=tr.steps_taken, actions=b.actions.clone(), logp=b.logp.clone(), xb=b.xb.clone(),
                    rewards=b.rewards.clone(), dones=b.dones.clone(), values=b.values[:T].clone())


def _pattern(name, shape, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random(shape) < 0.6).astype(F32)
    if name == 'chunk_zero':
        a[:T // MB] = 0.0       # the first minibatch has no active row
    elif name == 'all_zero':
        a[:] = 0.0
    return a


def _np(t):
    return t.detach().cpu().numpy()


def _check(tr, label, masked):
    """Everything finish_rollout produced, against float64 from the rollout's
    own rewards, values and done flags."""
    full, c = tr.buf, tr.cfg
    b = full if full.learner is None else full.learner
    A = b.A
    assert (A == len(LA)) == (full.learner is not None) and b.rewards.shape == (T, N, A)
    if full.learner is not None:
        # the dense rows are the learner's columns of the full buffers
        for name in ('rewards', 'logp', 'values'):
            dense, sel = getattr(b, name), getattr(full, name)[:, :, LA].contiguous()
            assert torch.equal(dense.view(torch.int32), sel.view(torch.int32)), name
        assert b.dones is full.dones
        if masked:
            assert torch.equal(b.active, full.active[:, :, LA])
    r, v, d = _np(b.rewards).reshape(T, -1), _np(b.values).reshape(T + 1, -1), _np(b.dones)
    assert np.all(np.isfinite(v)), 'values[horizon] not written'
    gamma, lam = float(F32(c.gamma)), float(F32(c.lam))
    ra, rr, ba, br = G.gae_ref_and_bound(r, v, d, gamma, lam, A)
    ret, adv = _np(b.ret).reshape(T, -1), _np(b.adv).reshape(T, -1)
    q_ret, _ = G.worst_ratio(ret, rr, br)
    # the statistics: the pre-normalisation adv is gone; ret - V recovers each
    # stored fp32 advantage to u |ret| (ret = fl(adv + V)), for this reference only
    n_el = adv.size
    w = _np(b.active).reshape(T, -1).astype(np.float64) if masked else np.ones_like(ra)
    a_rec = ret.astype(np.float64) - v[:T].astype(np.float64)
    s_ref, q_ref, n_ref = G.masked_stats_ref(a_rec, w)
    rec = U * np.abs(ret)
    fs = lambda x: math.fsum(np.ravel(x))  # noqa: E731
    # (fp64 sums of n_el terms in any order, + 4 for the norm's square root and square)
    e_sum = (n_el + 4) * 2.0 ** -53
    b_s = fs(w * rec) + e_sum * fs(w * np.abs(a_rec))
    b_q = fs(w * (2.0 * np.abs(a_rec) * rec + rec * rec)) + e_sum * q_ref
    stats = _np(b.adv_stats)
    q_s = abs(stats[0] - s_ref) / max(b_s, 1e-300) if stats[0] != s_ref else 0.0
    q_q = abs(stats[1] - q_ref) / max(b_q, 1e-300) if stats[1] != q_ref else 0.0
    assert stats[2] == n_ref == (max(float(w.sum()), 1.0) if masked else float(T * N * A)), (stats[2], n_ref)
    # adv: fp64 GAE, fp64 statistics of it, the header's normalisation; the bound composed of all three
    st_ref = G.masked_stats_ref(ra, w)
    d_s = fs(w * ba) + e_sum * fs(w * np.abs(ra))
    d_q = fs(w * (2.0 * np.abs(ra) * ba + ba * ba)) + e_sum * st_ref[1]
    ref = G.adv_norm_ref(ra, st_ref)
    bound = G.adv_norm_sensitivity(ra, st_ref, ba, d_s, d_q) + G.adv_norm_bound(ra, st_ref)
    q_adv, at = G.worst_ratio(adv, ref, bound)
    print(f'{label}: ret {q_ret:.3f} adv {q_adv:.3f} (worst at {divmod(at, ra.shape[1])}) stats {q_s:.3f} {q_q:.3f}'
          f' of their bounds; count {stats[2]:.0f}')
    for k, q in (('ret', q_ret), ('adv', q_adv), ('stats', max(q_s, q_q))):
        WORST[k] = max(WORST.get(k, 0.0), q)
    assert np.all(np.isfinite(adv))
    assert q_ret <= 1.0 and q_adv <= 1.0 and q_s <= 1.0 and q_q <= 1.0
    if masked:
        # row_w = active * rows / sum(active) per time chunk (zeros for an empty chunk), share = sum / rows
        wc = w.reshape(MB, -1)
        rows = wc.shape[1]
        n = wc.sum(1)
        f = np.where(n > 0, rows / np.maximum(n, 1.0), 0.0)
        w_ref, sh_ref = wc * f[:, None], n / rows
        got_w, got_sh = _np(b.row_w).reshape(MB, -1).astype(np.float64), _np(b.active_share).astype(np.float64)
        assert b.row_w.shape == b.active.shape and b.row_w.dtype == torch.float32
        assert np.all(np.abs(got_w - w_ref) <= U * w_ref) and np.all(np.abs(got_sh - sh_ref) <= U * sh_ref)
        assert np.all(got_w[n == 0] == 0.0)
    else:
        assert b.row_w is None
    return stats


def _unchanged(tr, keep):
    b = tr.buf
    assert tr.steps_taken == keep['steps'] == T
    for name in ('actions', 'logp', 'xb', 'rewards', 'dones'):
        assert torch.equal(getattr(b, name).view(torch.uint8), keep[name].view(torch.uint8)), name
    assert torch.equal(b.values[:T].view(torch.int32), keep['values'].view(torch.int32))


@pytest.mark.parametrize('form', [f for f in FORMS if f not in MASKED])
def test_finish_rollout_unmasked(form):
    tr, keep = _rolled(form)
    tr.finish_rollout()
    torch.cuda.synchronize()
    _check(tr, form, masked=False)
    _unchanged(tr, keep)


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('form', MASKED)
def test_finish_rollout_masked(form, pattern):
    tr, keep = _rolled(form)
    full = tr.buf
    full.active.copy_(torch.from_numpy(_pattern(pattern, tuple(full.active.shape), seed=len(pattern))))
    tr.finish_rollout()
    torch.cuda.synchronize()
    stats = _check(tr, f'{form} {pattern}', masked=True)
    _unchanged(tr, keep)
    b = full if full.learner is None else full.learner
    if pattern == 'all_zero':
        assert stats.tolist() == [0.0, 0.0, 1.0]            # the count clamped to 1
        assert not b.row_w.any() and not b.active_share.any()
    if pattern == 'chunk_zero':
        assert not b.row_w[:T // MB].any() and float(b.active_share[0]) == 0.0 and float(b.active_share[1]) > 0.0


@pytest.mark.parametrize('form', list(FORMS))
def test_bootstrap_row_is_a_fresh_act_call_on_the_last_row_block(form):
    """values[horizon]: the value output of act / act_x / act_sel on row block
    `horizon` with the current packed image, bit for bit (a wiring check)."""
    tr, keep = _rolled(form)
    tr.finish_rollout()
    torch.cuda.synchronize()
    full = tr.buf
    M = N * full.A
    acts = torch.zeros((M, 6), dtype=torch.int8, device='cuda')
    lp = torch.zeros((M,), device='cuda')
    val = torch.full((M,), float('nan'), device='cuda')
    if full.learner is not None:
        tr.fused.act_sel(full.xb[T], full.A, sum(1 << a for a in LA), tr.seed, 0, acts, lp, val)
    elif form == 'plain_obs':
        tr.fused.act(full.obs[T].view(-1, full.D), tr.seed, 0, acts, lp, val)
    else:
        tr.fused.act_x(full.xb[T], tr.seed, 0, acts, lp, val)
    torch.cuda.synchronize()
    got, fresh = full.values[T], val.view(N, full.A)
    if full.learner is not None:
        others = [a for a in range(full.A) if a not in LA]
        # (the other agents' rows are nobody's to write)
        assert bool(torch.isnan(got[:, others]).all()) and bool(torch.isnan(fresh[:, others]).all())
        got, fresh = got[:, LA].contiguous(), fresh[:, LA].contiguous()
        assert torch.equal(full.learner.values[T].view(torch.int32), got.view(torch.int32))
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.0
    assert torch.equal(got.contiguous().view(torch.int32), fresh.contiguous().view(torch.int32))
    _unchanged(tr, keep)


@pytest.mark.parametrize('form', ['plain_x', 'selfplay_mask'])
def test_equal_seeds_give_identical_bits(form):
    tr, _ = _rolled(form)
    other = _make(form)
    if tr.buf.active is not None:
        tr.buf.active.copy_(other.buf.active)   # (the masked cases above overwrote it)
    tr.finish_rollout()
    other.finish_rollout()
    torch.cuda.synchronize()
    b1 = tr.buf if tr.buf.learner is None else tr.buf.learner
    b2 = other.buf if other.buf.learner is None else other.buf.learner
    for name in ('adv', 'ret'):
        assert torch.equal(getattr(b1, name).view(torch.int32), getattr(b2, name).view(torch.int32)), name
    assert torch.equal(b1.adv_stats.view(torch.int64), b2.adv_stats.view(torch.int64))
    other.env.close()


def test_count_is_set_again_under_collectives(tmp_path):
    """With collectives the all-reduce sums the three statistics in place,
    the count among them; finish_rollout has to set this rank's count first,
    whatever the previous iteration's all-reduce left there."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group('gloo', init_method=f'file://{tmp_path / "rdzv"}', rank=0, world_size=1)
    try:
        tr = _make('plain_x', allreduce=True)
        assert tr.collectives and tr.world == 1
        b = tr.buf
        b.adv_stats[2] = 8.0 * T * N * b.A    # what an 8-rank all-reduce leaves in place
        tr.finish_rollout()
        torch.cuda.synchronize()
        _check(tr, 'plain_x, collectives', masked=False)
        assert float(b.adv_stats[2]) == float(T * N * b.A)
        tr.env.close()
    finally:
        dist.destroy_process_group()


def test_report_and_release():
    print('worst |d| / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))
    for form in FORMS:
        _rolled(form)[0].env.close()
    _rolled.cache_clear()
