"""The conservative pre-test of SolveTOI (toi_reject, csrc/mas_physics.h) at
its margin of 0.002 against the serial C oracle, which runs b2TimeOfImpact for
every (agent, static) pair and has no pre-test: a call the pre-test skips must
have returned alpha = 1, so nothing may differ.

2v2, 64 envs x 300 steps with every action held 40 steps, so agents push
against walls and boxes and rest or slide in contact -- the calls the margin
decides about (scripts/toi_pretest_probe.py) -- and the recorded wedged env
(tests/golden/wedged_2v2.npz), whose SolveTOI runs to the sub-step cap.

Bit-exact obs, reward and done every step, and per env the GPU's summed TOI
event count (env.set_toi_counter) equals the oracle's toi_event counter: a
skipped root-find that would have touched would lose an event."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from masurvival import abi  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival.config import C3_CONFIG, ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wedged_2v2.npz')
HI = np.array([3, 3, 3, 2, 2, 2])
N, T, HOLD = 64, 300, 40


def replay(seeds, actions):
    """The oracle on actions [T, n, A, 6], env by env (its counters are one
    set per thread): obs0 [n, A, D], obs [T, n, A, D], rew [T, n, A],
    done [T, n], TOI events and capped sub-steps per env."""
    rc = ResolvedConfig(C3_CONFIG)
    steps, n = actions.shape[:2]
    obs0, obs, rew, done, events, caps = [], [], [], np.zeros((steps, n), dtype=bool), [], []
    for e, seed in enumerate(seeds):
        ora = OracleEnv(rc.to_struct(), pcg64_state(int(seed)))
        obs0.append(ora.reset().copy())
        oracle.counters(True)
        oo, rr = [], []
        for t in range(steps):
            o, r, dn = ora.step(actions[t, e])
            if dn:
                o = ora.reset()
            oo.append(np.array(o, copy=True))
            rr.append(np.array(r, copy=True))
            done[t, e] = dn
        c = oracle.counters(True)
        events.append(c['toi_event'])
        caps.append(c['toi_cap'])
        obs.append(np.stack(oo))
        rew.append(np.stack(rr))
    return dict(seeds=[int(s) for s in seeds], actions=actions, obs0=np.stack(obs0), obs=np.stack(obs, 1),
                rew=np.stack(rew, 1), done=done, events=np.array(events), caps=np.array(caps))


@functools.lru_cache(maxsize=None)
def held_reference():
    rng = np.random.default_rng(40)
    a = np.empty((T, N, 4, 6), dtype=np.int8)
    for t in range(T):
        a[t] = rng.integers(0, HI, size=(N, 4, 6)) if t % HOLD == 0 else a[t - 1]
    return replay(range(N), a)


@functools.lru_cache(maxsize=None)
def wedged_reference():
    d = np.load(GOLDEN)
    a = d['actions'].astype(np.int8)
    return replay([int(d['env_seed'])] * 2, np.stack([a, a], 1))


def run_gpu(ref):
    n = len(ref['seeds'])
    try:
        env = VecMaSurvival(C3_CONFIG, n_envs=n, seeds=ref['seeds'], auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    toi_cnt = torch.zeros((n,), dtype=torch.int32, device=env.device)
    env.set_toi_counter(toi_cnt)
    assert np.array_equal(env.reset().cpu().numpy(), ref['obs0'])
    general = 0
    for t in range(ref['actions'].shape[0]):
        o, r, dn, _ = env.step(torch.as_tensor(ref['actions'][t], device=env.device))
        general += int((env.gen_flags() != 0).sum())
        assert np.array_equal(dn.cpu().numpy().astype(bool), ref['done'][t]), t
        assert np.array_equal(r.cpu().numpy(), ref['rew'][t]), t
        assert np.array_equal(o.cpu().numpy(), ref['obs'][t]), t
    toi = toi_cnt.cpu().numpy()
    env.set_toi_counter(None)
    assert env.invalid_actions() == 0
    env.close()
    caps, events = toi >> 16, toi & 0xffff
    print('GPU TOI events per env', events.tolist(), 'oracle', ref['events'].tolist(), 'general-path env steps',
          general)
    assert (ref['events'] < 65536).all()  # the counter's low half holds the sum
    assert np.array_equal(events, ref['events'])
    assert np.array_equal(caps > 0, ref['caps'] > 0)
    return general


def test_held_actions_match_oracle_and_count_the_same_toi_events():
    ref = held_reference()
    # the pushing agents make real TOI events, in many envs, and episodes end
    assert ref['events'].sum() > N and (ref['events'] > 0).sum() > N // 2
    general = run_gpu(ref)
    assert general > 0  # some env steps kept a pair past the pre-test


def test_wedged_replay_matches_oracle_and_counts_the_same_toi_events():
    ref = wedged_reference()
    assert (ref['caps'] > 0).all()  # the recording reaches the sub-step cap
    run_gpu(ref)
