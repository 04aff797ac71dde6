"""The repeated-event skip of toi_agent_group (csrc/mas_physics.h) against the
serial C oracle, on the recorded wedged 2v2 env (tests/golden/wedged_2v2.npz:
seed 8754 and 256 steps of policy actions; an agent wedged between statics,
whose SolveTOI runs to the sub-step cap, 18 TOI events per world step).

n_envs = 8: every env replays the recording, so one wave holds eight groups
that skip together.  n_envs = 9: env 8 takes uniform-random actions, so a
skipping group sits beside one that does not.  Both with the slow split off
and at its default (the wedged env moves to the slow list: both mappings of
the general-path list run the skip).

Bit-exact obs, reward and done every step, and per env the GPU's summed TOI
event count (env.set_toi_counter; the skipped events are counted, not
computed) equals the oracle's toi_event counter over the replay."""
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
OTHER_SEED = 8


@functools.lru_cache(maxsize=None)
def reference():
    """Oracle replays, computed once: the wedged env on the recorded actions
    and env OTHER_SEED on uniform-random ones.  Per env: seed, actions, obs
    after reset, per-step (obs, reward, done), the oracle's counters."""
    d = np.load(GOLDEN)
    rc = ResolvedConfig(C3_CONFIG)
    T = len(d['actions'])
    rnd = np.random.default_rng(OTHER_SEED).integers(0, HI, size=(T, rc.n_agents, 6)).astype(np.int8)
    out = []
    for seed, acts in ((int(d['env_seed']), d['actions'].astype(np.int8)), (OTHER_SEED, rnd)):
        ora = OracleEnv(rc.to_struct(), pcg64_state(seed))
        obs0 = ora.reset().copy()
        oracle.counters(True)
        steps = []
        for t in range(T):
            o, r, dn = ora.step(acts[t])
            if dn:
                o = ora.reset()
            steps.append((np.array(o, copy=True), np.array(r, copy=True), bool(dn)))
        out.append(dict(seed=seed, actions=acts, obs0=obs0, steps=steps, counters=oracle.counters(True)))
    assert [s[2] for s in out[0]['steps']] == [bool(x) for x in d['dones']]
    return tuple(out)


@pytest.mark.parametrize('split', [0, None], ids=['one-stream', 'default-split'])
@pytest.mark.parametrize('n', [8, 9])
def test_wedged_replay_matches_oracle_and_counts_skipped_events(n, split, monkeypatch):
    monkeypatch.delenv('MAS_SPLIT', raising=False)
    monkeypatch.delenv('MAS_SLOW_K', raising=False)
    wedged, other = reference()
    ref = [wedged] * 8 + [other] * (n - 8)
    try:
        env = VecMaSurvival(C3_CONFIG, n_envs=n, seeds=[r['seed'] for r in ref], auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    env.split_step(split)
    toi_cnt = torch.zeros((n,), dtype=torch.int32, device=env.device)
    env.set_toi_counter(toi_cnt)
    obs = env.reset().cpu().numpy()
    for e in range(n):
        assert np.array_equal(obs[e], ref[e]['obs0']), e
    side = 0
    for t in range(len(wedged['steps'])):
        a = np.stack([r['actions'][t] for r in ref])
        o, r, dn, _ = env.step(torch.as_tensor(a, device=env.device))
        o, r, dn = o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy()
        side += int((env.gen_flags() == 2).sum())
        for e in range(n):
            oo, rr, dd = ref[e]['steps'][t]
            assert bool(dn[e]) == dd and np.array_equal(r[e], rr), (t, e)
            assert np.array_equal(o[e], oo), (t, e)
    toi = toi_cnt.cpu().numpy()
    env.set_toi_counter(None)
    assert env.invalid_actions() == 0
    env.close()
    caps, events = toi >> 16, toi & 0xffff
    print('GPU TOI events per env', events.tolist(), 'capped agent world steps', caps.tolist(),
          'oracle', [(r['counters']['toi_event'], r['counters']['toi_cap']) for r in (wedged, other)],
          'slow-list env steps', side)
    for e in range(n):
        c = ref[e]['counters']
        assert c['toi_event'] < 65536  # the counter's low half holds the sum
        assert int(events[e]) == c['toi_event'], (e, int(events[e]), c['toi_event'])
        assert (caps[e] > 0) == (c['toi_cap'] > 0), (e, int(caps[e]), c['toi_cap'])
    # the recording reaches the sub-step cap, on both sides
    assert wedged['counters']['toi_cap'] > 0 and (caps[:8] > 0).all()
    if split is None:
        assert side > 0  # the wedged envs took the slow list
    else:
        assert side == 0
