"""TEST INFRASTRUCTURE: golden fixtures from RECORDED actions instead of a
scripted policy (make_golden.py's episodes draw their actions from a seed).

Runs the reference's own Python over the shim exactly as make_golden.py does
(its load_reference / flatten_obs / max_inventory are used as they are) and
writes a fixture with the same fields, plus `dones`: `done` as uint8, the
name and type the replay tests of the recording read.

  wedged_2v2  the PPO-regime 2v2 env with an agent wedged between statics,
              whose SolveTOI runs to Box2D's sub-step cap: seed and 256 steps
              of trained-policy actions of profiles/r02_wedged_env.npz (no
              episode end).

Usage:  python tests/golden/make_golden_recorded.py   (needs the reference, as make_golden.py)
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import Box2D  # noqa: E402  (the shim)

RECORDED = [
    # name, config, recording (env_seed, actions [T, A, 6]) relative to the repository root
    ('wedged_2v2', {'agents': {'n_agents': 4, 'agent_size': 1}, 'teams': {'twoteams': True}, 'melee': mg.MELEE},
     'profiles/r02_wedged_env.npz'),
]


def run_recorded(mod, name, config, env_seed, actions):
    env = mod.MaSurvival(config=copy.deepcopy(config))
    groups = env.simulation.groups
    Box2D.CANONICAL_GROUPS[:] = list(groups.values())
    Box2D.STATIC_GROUPS[:] = [groups['walls'], groups['boxes']]
    env.np_random = np.random.default_rng(env_seed)
    flat0, keys = mg.flatten_obs(env.reset())
    obs_l, act_l, rew_l, done_l = [flat0], [], [], []
    max_inv = 0
    for t in range(len(actions)):
        acts = tuple(np.asarray(a) for a in actions[t])
        obs, rew, done, info = env.step(acts)
        obs_l.append(mg.flatten_obs(obs)[0])
        act_l.append(np.stack(acts).astype(np.int8))
        rew_l.append(np.asarray(rew, dtype=np.float32))
        done_l.append(bool(done))
        max_inv = max(max_inv, mg.max_inventory(env))
        if done:
            break
    stats = env.flush_stats()
    done_a = np.array(done_l, dtype=np.bool_)
    return dict(
        name=name,
        config=json.dumps(config),
        env_seed=env_seed,
        act_seed=0,
        keys=json.dumps(keys),
        obs=np.stack(obs_l).astype(np.float32),
        actions=np.stack(act_l),
        rewards=np.stack(rew_l),
        done=done_a,
        dones=done_a.astype(np.uint8),
        stats=json.dumps({k: float(v) for k, v in stats.items()}),
        max_inventory=np.int32(max_inv),
    )


def main(only=None):
    for name, config, rel in RECORDED:
        if only and name not in only:
            continue
        rec = np.load(os.path.join(HERE, '..', '..', rel))
        mod = mg.load_reference()  # a fresh import per episode, as make_golden.main
        d = run_recorded(mod, name, config, int(rec['env_seed']), rec['actions'].astype(np.int8))
        out = os.path.join(HERE, name + '.npz')
        np.savez_compressed(out, **d)
        print(f"{name}: steps={len(d['done'])} done={bool(d['done'][-1])} stats={d['stats']} "
              f"-> {os.path.getsize(out) // 1024} KiB", flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
