"""The env step's rarely taken code paths, bit for bit against the oracle at
every step: 2v2, 40 envs with auto-reset (two full 16-env k_post_lanes waves
and a partial one; five 8-env k_gen_solve_g waves), seeded uniform-random
actions, long enough that every env finishes an episode and is reset in
place at least once and that an agent dies holding an item (DeathDrop's RNG
draws and spawns) -- asserted from the oracle's own outputs, so the test
fails rather than passes if the run stops covering them.  Run once on the
usual routing (contact-free fast path, general path for the envs that leave
it) and once with every env forced onto the general path, where each env
takes both world steps of k_gen_solve_g's world-step loop; and, in a fresh
child process (the variable is read once per process), with
MAS_GEN_FUSE2=0: one k_gen_solve_g launch per world step.

Compared per step: obs, rewards, done flags and the flushed stats
(np.array_equal: the kernels restate the oracle's float op order, tolerance 0).

Seeds and length were picked on the CPU with the oracle: env seeds 0..39 with
slots 4 and 14 re-seeded (84, 294: an agent of each dies with an item in its
inventory, by steps 300 / 250); the last env's first reset is at step 524 of
the 560 run here."""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import golden_replay as gr  # noqa: E402
import oracle as ora  # noqa: E402
from masurvival import abi  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival.config import C3_CONFIG, ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, T_CHILD = 40, 560, 64
SEEDS = [84 if e == 4 else 294 if e == 14 else e for e in range(N)]
HI = np.array([3, 3, 3, 2, 2, 2])


@lru_cache(maxsize=None)
def reference(steps):
    """The oracle's run, computed once and shared read-only: actions
    [steps, N, A, 6], obs0 [N, A, D], per step obs / rewards / done / flushed
    stats, each env's reset count and the oracle's coverage counters."""
    rc = ResolvedConfig(C3_CONFIG)
    ors = [OracleEnv(rc.to_struct(), pcg64_state(s)) for s in SEEDS]
    obs0 = np.stack([o.reset() for o in ors])
    ora.counters()  # (zeroed)
    rng = np.random.default_rng(N)
    acts = np.stack([rng.integers(0, HI, size=(N, rc.n_agents, 6)).astype(np.int8) for _ in range(steps)])
    obs = np.zeros((steps,) + obs0.shape, np.float32)
    rew = np.zeros((steps, N, rc.n_agents), np.float32)
    done = np.zeros((steps, N), bool)
    stats = np.zeros((steps, N, 19), np.float32)
    resets = np.zeros(N, int)
    for t in range(steps):
        for e, o in enumerate(ors):
            oo, rr, dd = o.step(acts[t, e])
            if dd:
                oo = o.reset()
                resets[e] += 1
            obs[t, e], rew[t, e], done[t, e] = oo, rr, dd
            stats[t, e] = o.flush_stats()
    cnt = ora.counters()
    for a in (acts, obs0, obs, rew, done, stats, resets):
        a.setflags(write=False)
    return acts, obs0, obs, rew, done, stats, resets, cnt


def run_gpu(steps, forced):
    """Steps the GPU env through the reference's actions; asserts every step's
    outputs equal the oracle's."""
    acts, obs0, obs, rew, done, stats, _, _ = reference(steps)
    try:
        env = VecMaSurvival(C3_CONFIG, n_envs=N, seeds=SEEDS, auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    if forced:
        env.force_general(True)
    assert np.array_equal(env.reset().cpu().numpy(), obs0)
    a_dev = torch.as_tensor(acts.copy(), device=env.device)  # (the shared reference is read-only)
    got = []
    for t in range(steps):
        o, r, dn, _ = env.step(a_dev[t])
        got.append((o.clone(), r.clone(), dn.clone(), env.flush_stats()))
        if forced:
            assert env.debug_counters()['phys_general_envs'] == N, t
    for t, (o, r, dn, s) in enumerate(got):
        o, r, dn, s = o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy().astype(bool), s.cpu().numpy()
        assert np.array_equal(dn, done[t]), (t, np.nonzero(dn != done[t])[0])
        assert np.array_equal(r, rew[t]), (t, np.nonzero((r != rew[t]).any(1))[0])
        for e in range(N):
            assert np.array_equal(o[e], obs[t, e]), (t, e, gr.diff(o[e], obs[t, e]))
        assert np.array_equal(s, stats[t]), (t, np.nonzero((s != stats[t]).any(1))[0])
    assert env.debug_guards()['list_overflow'] == 0
    env.close()


def test_reference_run_covers_reset_and_death_drop():
    """Every env was reset in place at least once, and at least one agent died
    with an item to drop (the oracle's drop_items counter: items dropped by
    DeathDrop)."""
    *_, resets, cnt = reference(T)
    assert resets.min() >= 1, np.nonzero(resets == 0)[0]
    assert cnt['drop_items'] >= 1, cnt


@pytest.mark.parametrize('forced', [False, True], ids=['routed', 'forced_general'])
def test_every_step_matches_oracle(forced):
    run_gpu(T, forced)


def test_one_launch_per_world_step_in_child_process():
    """MAS_GEN_FUSE2=0 (k_gen_solve_g once per world step: the loop's
    one-iteration form), every env forced onto the general path."""
    path = [os.path.join(ROOT, d) for d in ('tests', 'oracle', 'gym-ma-survival-2d_amd')]  # (as conftest.py)
    env = dict(os.environ, MAS_GEN_FUSE2='0',
               PYTHONPATH=os.pathsep.join(path + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], capture_output=True, text=True, env=env,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert 'child ok' in r.stdout, r.stdout[-2000:]


if __name__ == '__main__' and sys.argv[1:] == ['child']:
    assert os.environ.get('MAS_GEN_FUSE2') == '0'
    run_gpu(T_CHILD, True)
    print('child ok')
