"""PPOTrainer._update_fused observed call by call: 2v2 x 64 envs, horizon 8,
4 minibatches, 2 epochs, so eight minibatches of 2 * 64 * 4 = 512 rows.  The
trainer's FusedPolicy.grads, FusedAdam.step and FusedPolicy.pack are wrapped
with recorders that call through; nothing of the update is re-implemented.

Checked: every time chunk once per epoch, in the order of the seeded
permutation; each call's tensors are exactly the chunk's slices of the rollout
buffer (pointer and shape), row_w included with mask_dead; the packed image at
every grads call is byte-equal to the image a second FusedPolicy packs from the
parameters as they are then (a pack follows every step); every gradient is
the fp64 sum over the rows the call stored (policy_rows_ref.check_grads) and
is what the step then reads; the fused kernel's layer 3, which stores neither
h2 nor dz, is held to the h2 and dz the unfused kernel stores for the same
rows once that kernel's h1, dA1 and dA2 equal the fused call's bit for bit:
check_grads on their sums and check_dw3 teacher-forced on that h2 (unforced,
a rollout's rows cross clip boundaries: check_dw3's docstring; the unforced
figure is printed beside the asserted ones); every step
is adam_ref's (update_ref.check_adam); stats only on the last call, and
last_stats are that call's partials; the next rollout's first rows are the
last rollout's final ones."""
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import policy_rows_ref as R  # noqa: E402
import test_gpu_policy_rows as TR  # noqa: E402
import test_gpu_policy_rows_w as TRW  # noqa: E402
import update_ref as UR  # noqa: E402
from masurvival import ppo as ppo_mod  # noqa: E402
from masurvival.config import C3_CONFIG  # noqa: E402
from masurvival.ppo import FusedPolicy, PPOConfig, PPOTrainer  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402

N, T, MB, EPOCHS = 64, 8, 4, 2


def _np(t):
    return t.detach().cpu().numpy().copy()


def _shadow(fp, xb, batch, cf, row_w):
    """What the unfused train kernel stores for this minibatch and fp's packed
    image, on sentinel buffers of the trainer's row stride ([M, F] fp32): the
    h2 and dz the fused kernel (mas_policy_train_dw3) keeps to itself."""
    M = xb.shape[0]
    B = TR.Buffers(fp.lib, M, False)
    assert B.ld == fp._bufs['ld']
    if row_w is None:
        B.run(fp, xb, batch, cf)
    else:
        TRW._run(B, fp, xb, batch, cf, row_w)
    assert B.untouched() == []
    return B.outputs(fp)


@pytest.mark.parametrize('mask_dead', [False, True])
def test_update_fused_call_by_call(mask_dead, monkeypatch):
    for k in ('MAS_POL_DB', 'MAS_POL_CW', 'MAS_POL_FORCE_OFF64', 'MAS_POL_DW3'):
        monkeypatch.delenv(k, raising=False)
    env = VecMaSurvival(C3_CONFIG, n_envs=N, seeds=range(N), auto_reset=True)
    cfg = PPOConfig(horizon=T, minibatches=MB, epochs=EPOCHS, mask_dead=mask_dead)
    tr = PPOTrainer(env, cfg, seed=0)
    assert tr.fused is not None and tr.fused_opt is not None and tr.fused.layout == 'fm' and not tr.collectives
    for t in range(T):
        tr.rollout_step(t)
    tr.finish_rollout()
    torch.cuda.synchronize()
    b, fp, fa = tr.buf, tr.fused, tr.fused_opt
    D, Dx, dev = fp.D, fp.Dx, tr.device
    tc = T // MB
    M = tc * b.N * b.A
    assert M == 512
    cf = (cfg.clip, cfg.vf_coef, cfg.ent_coef, 1.0 / M)
    grp = tr.opt.param_groups[0]
    events, calls, steps = [], [], []
    o_grads, o_step, o_pack = fp.grads, fa.step, fp.pack

    def grads(xb, actions, old_logp, adv, ret, c, stats=True, row_w=None):
        assert c is cfg
        # the image the kernels are about to read against a fresh pack of the parameters as they are now
        fresh = FusedPolicy(tr.policy, D, dev)
        fresh.pack()
        torch.cuda.synchronize()
        rec = dict(stats=stats, fresh=bool(torch.equal(fp.packed, fresh.packed)),
                   args={k: (t.data_ptr(), tuple(t.shape), t.dtype) for k, t in
                         (('xb', xb), ('actions', actions), ('logp', old_logp), ('adv', adv), ('ret', ret))},
                   row_w=None if row_w is None else (row_w.data_ptr(), tuple(row_w.shape), row_w.dtype))
        P = R.params(tr.policy)
        st = o_grads(xb, actions, old_logp, adv, ret, c, stats=stats, row_w=row_w)
        torch.cuda.synchronize()
        B = fp._bufs
        out = {k: B[k][:256, :M].T.float() for k in ('h1', 'h2', 'da1', 'da2') if k in B}
        if 'dz' in B:
            out['dz'] = B['dz'][:, :M].T.float()
        g = {k: q.grad for k, q in zip(R.GRADS, tr.policy.parameters())}
        res = R.check_grads(xb[:, :D + 1], out, g, gemm=(1,), chunks=ppo_mod._split_k(M))
        if 'h2' not in out:
            # the fused kernel stored neither h2 nor dz: the unfused kernel's, once its other tensors are the
            # fused call's bit for bit; then layer 3 against their fp64 sums (check_grads) and against the loss
            # gradient at the logits of that h2 (check_dw3, teacher-forced)
            batch = (actions, old_logp, adv, ret)
            sh = _shadow(fp, xb, batch, cf, row_w)
            for k in ('h1', 'da1', 'da2'):
                assert torch.equal(sh[k], out[k]), (k, 'the unfused kernel stored other rows than the fused one')
            r3 = R.check_dw3(P, xb[:, :D], batch, cf, g['w3'], g['b3'], row_w=row_w, h2k=sh['h2'])
            rows = R.check_grads(xb[:, :D + 1], dict(out, h2=sh['h2'], dz=sh['dz']), g, gemm=(1,),
                                 chunks=ppo_mod._split_k(M))
            un = R.check_dw3(P, xb[:, :D], batch, cf, g['w3'], g['b3'], row_w=row_w)
            z_un = R.forward(P, xb[:, :D])[2]
            z_k = sh['h2'].double() @ P['W3'].T + P['b3']
            s_un = R.loss_rows(z_un, *batch, *cf, row_w=row_w)
            s_k = R.loss_rows(z_k, *batch, *cf, row_w=row_w)
            crossed = int(((s_un['s1'] <= s_un['ratio'].clamp(1 - cfg.clip, 1 + cfg.clip) * adv.double())
                           != (s_k['s1'] <= s_k['ratio'].clamp(1 - cfg.clip, 1 + cfg.clip) * adv.double())).sum())
            res.update(w3=r3['dw3'], b3=r3['db3'], w3_rows=rows['w3'], b3_rows=rows['b3'], flip_rows=r3['flip_rows'],
                       w3_unforced=un['dw3'], b3_unforced=un['db3'], crossed=crossed,
                       dlogratio=float((R.log_prob(z_un, actions) - R.log_prob(z_k, actions)).abs().max()))
        rec.update(res=res, st=st, part=B['part'].clone(), g=fa.g.clone())
        calls.append(rec)
        events.append('grads')
        return st

    def step(max_norm, grad_scale=1.0):
        torch.cuda.synchronize()
        before = [_np(t) for t in (fa.p, fa.g, fa.m, fa.v)]
        o_step(max_norm, grad_scale)
        torch.cuda.synchronize()
        steps.append(dict(max_norm=max_norm, grad_scale=grad_scale, before=before, g_dev=fa.g.clone(),
                          after=[_np(t) for t in (fa.p, fa.m, fa.v)],
                          step=[float(tr.opt.state[q]['step']) for q in tr.policy.parameters()]))
        events.append('step')

    def pack():
        o_pack()
        events.append('pack')

    monkeypatch.setattr(fp, 'grads', grads)
    monkeypatch.setattr(fa, 'step', step)
    monkeypatch.setattr(fp, 'pack', pack)
    # every parameter in the order check_grads names them, and FusedAdam's spans in that order
    assert [n for n, _ in tr.policy.named_parameters()] == ['body.0.weight', 'body.0.bias', 'body.2.weight',
                                                             'body.2.bias', 'head.weight', 'head.bias']
    order = torch.randperm(MB, generator=torch.Generator().manual_seed(tr.steps_taken)).tolist()
    last_rows = b.xb[T].clone() if tr.x_obs else None
    tr.update()
    torch.cuda.synchronize()

    assert len(calls) == MB * EPOCHS == 8 and len(steps) == 8
    visited = []
    for i, rec in enumerate(calls):
        ks = [k for k in range(MB) if rec['args']['xb'][0] == b.xb[k * tc].data_ptr()]
        assert len(ks) == 1, (i, 'xb is no time chunk of the buffer')
        k = ks[0]
        visited.append(k)
        sl = slice(k * tc, (k + 1) * tc)
        want = {'xb': (b.xb[sl], (M, Dx), torch.bfloat16), 'actions': (b.actions[sl], (M, 6), torch.int8),
                'logp': (b.logp[sl], (M,), torch.float32), 'adv': (b.adv[sl], (M,), torch.float32),
                'ret': (b.ret[sl], (M,), torch.float32)}
        for name, (t, shape, dt) in want.items():
            assert rec['args'][name] == (t.data_ptr(), shape, dt), (i, name)
        if mask_dead:
            assert rec['row_w'] == (b.row_w[sl].data_ptr(), (M,), torch.float32), i
        else:
            assert rec['row_w'] is None
        assert rec['stats'] == (i == 7), i
        assert (rec['st'] is None) == (i != 7)
        assert rec['fresh'], f'grads call {i}: the packed image is not the pack of the current parameters'
        print(f'update mask_dead={mask_dead} call {i} chunk {k}: '
              + ' '.join(f'{n} {rec["res"][n]:.3f}' for n in R.GRADS)
              + f' | w1 over the fp32-only bound {rec["res"]["w1_x_fp32"]:.1f}'
              + ''.join(f' {n} {rec["res"][n]:.3g}' for n in ('w3_rows', 'b3_rows', 'flip_rows', 'w3_unforced',
                                                              'b3_unforced', 'crossed', 'dlogratio')
                        if n in rec['res']))
        for n in R.GRADS + tuple(n for n in ('w3_rows', 'b3_rows') if n in rec['res']):
            assert rec['res'][n] <= 1.0, (i, n, rec['res'])
    assert events == ['grads', 'step', 'pack'] * 8
    assert visited == order * EPOCHS, (visited, order)
    for e in range(EPOCHS):
        assert sorted(visited[e * MB:(e + 1) * MB]) == list(range(MB))

    for i, s in enumerate(steps):
        assert s['max_norm'] == cfg.max_grad_norm and s['grad_scale'] == 1.0
        assert s['step'] == [float(i + 1)] * 6
        assert torch.equal(s['g_dev'], calls[i]['g']), (i, 'the step read another gradient than grads left')
        p0, g0, m0, v0 = s['before']
        res = UR.check_adam(p0, g0, m0, v0, 1.0, cfg.max_grad_norm, grp['lr'], grp['betas'], grp['eps'], i + 1,
                            *s['after'])
        print(f'update mask_dead={mask_dead} step {i + 1}: ' + ' '.join(f'{n} {res[n]:.3f}' for n in 'pmv'))
        for n in 'pmv':
            assert res[n] <= 1.0, (i, n, res)
        if i + 1 < len(steps):  # nothing else moved the parameters or the moments
            nb = steps[i + 1]['before']
            for a, c in zip(s['after'], (nb[0], nb[2], nb[3])):
                assert (a == c).all()

    want = FusedPolicy._loss_stats(calls[7]['part'], M, cfg)
    for key, w in zip(('loss', 'pg', 'v', 'entropy', 'clipfrac'), want):
        assert torch.equal(tr.last_stats[key], w), key
    # the image after the update is the pack of the final parameters
    fresh = FusedPolicy(tr.policy, D, dev)
    fresh.pack()
    assert torch.equal(fp.packed, fresh.packed)
    if tr.x_obs:
        assert torch.equal(b.xb[0], b.xb[T]) and torch.equal(b.xb[T], last_rows)
    env.close()
