"""Self-play on the fused path of PPOTrainer (opponent= / learner_agents=) on
the 2v2 env: two act_sel calls per step fill one actions buffer, the learner's
rows are compacted by mas_rows_select, and GAE, the advantage normalisation
and the update run on the dense rows alone.

T = 8, two minibatches, fixed env seeds.  Every check runs at N = 64 (512
learner rows per minibatch: the mas_policy_train_dw3 path) and at N = 24 (192
rows: the unfused mas_policy_train_ld + mas_policy_dw fallback)."""
import copy
import json
import os

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import ppo as ppo_mod  # noqa: E402
from masurvival.match import Match, load_policy  # noqa: E402
from masurvival.ppo import FusedPolicy, PolicyMLP, PPOConfig, PPOTrainer, policy_loss_reference  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'configs', '2v2.json')) as _f:
    CFG_2V2 = json.load(_f)
T, MB = 8, 2
SIZES = [64, 24]
LA = [0, 1]


def _env(n, first_seed=0):
    return VecMaSurvival(CFG_2V2, n_envs=n, seeds=range(first_seed, first_seed + n), auto_reset=True)


def _cfg(**kw):
    return PPOConfig(horizon=T, minibatches=MB, **kw)


def _opponent(D, seed=77):
    torch.manual_seed(seed)
    return PolicyMLP(D, 256)


def _same(ps, qs):
    ps, qs = list(ps), list(qs)
    return len(ps) == len(qs) and all(torch.equal(p, q) for p, q in zip(ps, qs))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rollout(tr):
    for t in range(T):
        tr.rollout_step(t)
    tr.finish_rollout()


def _used_dw3(tr):
    return 'h2' not in tr.fused._bufs  # only the unfused path stores h2 / dz


@pytest.mark.parametrize('n', SIZES)
def test_full_learner_set_is_the_plain_trainer(n):
    plain = PPOTrainer(_env(n), _cfg(), seed=0)
    sel = PPOTrainer(_env(n), _cfg(), seed=0, learner_agents=[0, 1, 2, 3])
    assert plain.buf.learner is None and sel.buf.learner is not None and sel.opponent is None
    for _ in range(2):
        plain.iteration()
        sel.iteration()
    torch.cuda.synchronize()
    assert _same(plain.policy.parameters(), sel.policy.parameters())
    s1, s2 = plain.opt.state_dict()['state'], sel.opt.state_dict()['state']
    for k in s1:
        assert torch.equal(s1[k]['exp_avg'], s2[k]['exp_avg']) and torch.equal(s1[k]['exp_avg_sq'], s2[k]['exp_avg_sq'])
    assert torch.equal(plain.buf.xb, sel.buf.xb)
    plain.env.close()
    sel.env.close()


@pytest.mark.parametrize('n', SIZES)
def test_same_weights_on_both_sides_is_the_plain_rollout(n):
    plain = PPOTrainer(_env(n), _cfg(), seed=0)
    sp = PPOTrainer(_env(n), _cfg(), seed=0, opponent=copy.deepcopy(plain.policy), learner_agents=LA)
    assert sp.learner_agents == LA and _same(sp.opponent.parameters(), plain.policy.parameters())
    _rollout(plain)
    _rollout(sp)
    torch.cuda.synchronize()
    b0, b, lb = plain.buf, sp.buf, sp.buf.learner
    A, m, Dx = b.A, len(LA), sp.fused.Dx
    for name in ('actions', 'rewards', 'dones'):
        assert torch.equal(getattr(b0, name), getattr(b, name)), name
    assert torch.equal(b0.xb, b.xb)
    assert torch.equal(_bits(b0.logp[:, :, LA]), _bits(b.logp[:, :, LA]))
    assert torch.equal(_bits(b0.values[:, :, LA]), _bits(b.values[:, :, LA]))  # the bootstrap row included
    # the dense buffers are torch indexing of the full ones
    assert torch.equal(_bits(lb.xb), _bits(b.xb[:T].view(T, n, A, Dx)[:, :, LA].reshape(T, n * m, Dx)))
    assert torch.equal(lb.actions, b.actions[:, :, LA])
    for name in ('logp', 'rewards', 'values'):
        assert torch.equal(_bits(getattr(lb, name)), _bits(getattr(b, name)[:, :, LA])), name
    assert float(lb.adv_stats[2]) == T * n * m
    # adv / ret: mas_gae on torch-gathered inputs (n_agents = m), then the normalisation
    c = sp.cfg
    adv, ret = torch.empty_like(lb.adv), torch.empty_like(lb.ret)
    stats = torch.zeros((3,), dtype=torch.float64, device=b.adv.device)
    stats[2] = float(T * n * m)
    ppo_mod.gae(b.rewards[:, :, LA].contiguous(), b.values[:, :, LA].contiguous(), b.dones, c.gamma, c.lam, adv, ret,
                stats[:2], m)
    ppo_mod.adv_normalize(adv, stats)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lb.ret), _bits(ret)) and torch.equal(_bits(lb.adv), _bits(adv))
    assert torch.equal(lb.adv_stats, stats)
    plain.env.close()
    sp.env.close()


@pytest.mark.parametrize('n', SIZES)
def test_update_leaves_the_opponent_alone_and_it_keeps_playing(n):
    env = _env(n)
    opp = _opponent(env.obs_dim)
    sp = PPOTrainer(env, _cfg(), seed=0, opponent=opp, learner_agents=LA)
    image = sp.opp_fused.packed.clone()
    before = [p.detach().clone() for p in sp.policy.parameters()]
    learner_image = sp.fused.packed.clone()
    _rollout(sp)
    sp.update()
    torch.cuda.synchronize()
    assert _used_dw3(sp) == (n == 64)  # 512 rows: the dw3 path; 192 rows: the fallback
    assert torch.equal(sp.opp_fused.packed, image)
    assert _same(sp.opponent.parameters(), [p.to(env.device) for p in opp.parameters()])
    assert not _same(sp.policy.parameters(), before) and not torch.equal(sp.fused.packed, learner_image)
    # the next rollout: the opponent's rows of actions[t] are a fresh act_sel of the opponent on the stored rows
    step0 = sp.steps_taken
    _rollout(sp)
    fresh = FusedPolicy(copy.deepcopy(opp).to(env.device), env.obs_dim, env.device)
    fresh.pack()
    b = sp.buf
    M = n * b.A
    others = [a for a in range(b.A) if a not in LA]
    omask = sum(1 << a for a in others)
    for t in range(T):
        acts = torch.full((M, 6), -7, dtype=torch.int8, device=env.device)
        lp, v = torch.empty((M,), device=env.device), torch.empty((M,), device=env.device)
        fresh.act_sel(b.xb[t], b.A, omask, sp.seed, step0 + t, acts, lp, v)
        assert torch.equal(b.actions[t][:, others], acts.view(n, b.A, 6)[:, others]), t
    env.close()


def _cos(a, b):
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize('n', SIZES)
def test_first_minibatch_gradient_matches_the_torch_reference(n):
    """FusedPolicy.grads on the dense rows of the first minibatch against
    policy_loss_reference on the learner rows of the full buffers (bf16-rounded
    weights, fp32 arithmetic); the bounds of tests/test_gpu_policy.py:
    cosine >= 0.999 and norms within 3 % per parameter tensor."""
    env = _env(n)
    sp = PPOTrainer(env, _cfg(), seed=0, opponent=_opponent(env.obs_dim), learner_agents=LA)
    _rollout(sp)
    b, lb, c = sp.buf, sp.buf.learner, sp.cfg
    A, m, D, Dx = b.A, len(LA), b.D, sp.fused.Dx
    tc = T // MB
    M = tc * n * m
    sp.fused.grads(lb.xb[:tc].reshape(M, Dx), lb.actions[:tc].reshape(M, 6), lb.logp[:tc].reshape(M),
                   lb.adv[:tc].reshape(M), lb.ret[:tc].reshape(M), c)
    torch.cuda.synchronize()
    assert _used_dw3(sp) == (n == 64)
    ref = copy.deepcopy(sp.policy)
    with torch.no_grad():
        for prm in ref.parameters():
            prm.copy_(prm.bfloat16().float())
            prm.grad = None
    x = b.xb[:tc].view(tc, n, A, Dx)[:, :, LA, :D].float().reshape(M, D)
    rl = policy_loss_reference(ref, x, b.actions[:tc][:, :, LA].reshape(M, 6), b.logp[:tc][:, :, LA].reshape(M),
                               lb.adv[:tc].reshape(M), lb.ret[:tc].reshape(M), c)[0]
    rl.backward()
    for (name, a), r in zip(sp.policy.named_parameters(), ref.parameters()):
        ga, gb = a.grad.float(), r.grad
        cos, rel = _cos(ga, gb), float((ga.norm() - gb.norm()).abs() / gb.norm())
        print(f'n={n} {name}: cosine {cos:.6f} norm error {rel:.4%}')
        assert cos >= 0.999, (name, cos)
        assert rel <= 0.03, (name, rel)
    env.close()


@pytest.mark.parametrize('n', SIZES)
def test_checkpoint_round_trip_and_match(tmp_path, n):
    """save after an iteration, load into a fresh trainer on a fresh env: the
    next rollout is bit-identical to the run that never stopped, the opponent
    included; the checkpoint then plays a Match against its opponent."""
    env = _env(n)
    sp = PPOTrainer(env, _cfg(), seed=0, opponent=_opponent(env.obs_dim), learner_agents=LA)
    sp.iteration()
    path = str(tmp_path / 'selfplay.pt')
    sp.save(path)
    env2 = _env(n, first_seed=1000)
    sp2 = PPOTrainer(env2, _cfg(), seed=5, opponent=_opponent(env.obs_dim, seed=78), learner_agents=LA)
    assert not _same(sp2.opponent.parameters(), sp.opponent.parameters())
    sp2.load(path)
    assert _same(sp2.opponent.parameters(), sp.opponent.parameters())
    assert torch.equal(sp2.opp_fused.packed, sp.opp_fused.packed)
    for tr in (sp, sp2):
        for t in range(T):
            tr.rollout_step(t)
    torch.cuda.synchronize()
    b1, b2 = sp.buf, sp2.buf
    assert torch.equal(b1.xb, b2.xb)
    for name in ('actions', 'rewards', 'dones'):
        assert torch.equal(getattr(b1, name), getattr(b2, name)), name
    assert torch.equal(_bits(b1.logp[:, :, LA]), _bits(b2.logp[:, :, LA]))
    assert torch.equal(_bits(b1.values[:T][:, :, LA]), _bits(b2.values[:T][:, :, LA]))
    with pytest.raises(ValueError, match='learner_agents'):
        PPOTrainer(env2, _cfg(), seed=5, opponent=_opponent(env.obs_dim), learner_agents=[0, 2]).load(path)
    env.close()
    env2.close()
    # 'policy' is the learner, 'opponent' its opponent: both load as any checkpoint's policy
    sd = torch.load(path, map_location='cpu', weights_only=True)
    assert sd['learner_agents'] == LA and sd['iterations'] == 1
    learner, opp = load_policy(path, 'cuda'), load_policy({'policy': sd['opponent']}, 'cuda')
    menv = _env(n)
    res = Match(menv, [learner, opp], seed=1).run(steps=16)
    assert isinstance(res, dict) and res['steps'] == 16
    assert {'episodes', 'wins', 'draws', 'return', 'mean_length'} <= set(res) and len(res['wins']) == 2
    menv.close()


def test_gpu_selfplay_needs_the_x_obs_fused_unsharded_path():
    from masurvival.vec_env import ShardedVecMaSurvival
    env = _env(8)
    opp = _opponent(env.obs_dim)
    with pytest.raises(ValueError, match='fused'):
        PPOTrainer(env, _cfg(fused=False), seed=0, opponent=opp)
    with pytest.raises(ValueError, match='x_obs'):
        PPOTrainer(env, _cfg(x_obs=False), seed=0, opponent=opp)
    env.close()
    sh = ShardedVecMaSurvival(CFG_2V2, n_envs=8, shards=2, seeds=range(8), auto_reset=True)
    with pytest.raises(ValueError, match='unsharded'):
        PPOTrainer(sh, _cfg(), seed=0, opponent=opp)
    sh.close()
