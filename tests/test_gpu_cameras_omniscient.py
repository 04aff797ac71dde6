"""The camera pass under omniscient observations (cameras_v, csrc/
mas_post_lanes.h; update_seen and update_seen_dealt, csrc/mas_step.h): only
the other live agents are line-of-sight candidates there, because the
observation reads `seen` for others_mask alone; boxes, items, heals and walls
still occlude.  A config with observation.omniscent = False keeps every
candidate.

Omniscient 2v2 and FFA4 (heals, randomized boxes) and the non-omniscient
last-alive config of tests/golden (nonomni_lastalive_s7), 32 envs x 300 steps
of uniform-random actions with auto-reset: obs, reward and done bit for bit
against the serial C oracle, which casts every ray; agents die, episodes end
and reset in place, others_mask holds both values; a mas_step_x twin on the
same seeds and actions ends with the same state image."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from masurvival import abi  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival.config import C3_CONFIG, C5_CONFIG, ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402

HI = np.array([3, 3, 3, 2, 2, 2])
N, T = 32, 300
NONOMNI = {'agents': {'n_agents': 4, 'agent_size': 1}, 'observation': {'omniscent': False},
           'gameover': {'mode': 'lastalive'}, 'melee': {'range': 2, 'damage': 20, 'cooldown': 40, 'drift': True}}
CONFIGS = {'2v2': (C3_CONFIG, True), 'ffa4': (C5_CONFIG, True), 'nonomni': (NONOMNI, False)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's replay, computed once per config: actions [T, N, A, 6],
    obs0 [N, A, D], obs [T, N, A, D], rew [T, N, A], done [T, N]."""
    cfg, omni = CONFIGS[name]
    rc = ResolvedConfig(cfg)
    assert bool(rc.to_struct().omniscient) == omni
    A = rc.n_agents
    actions = np.random.default_rng(len(name)).integers(0, HI, size=(T, N, A, 6)).astype(np.int8)
    obs0, obs, rew, done = [], [], [], np.zeros((T, N), dtype=bool)
    for e in range(N):
        ora = OracleEnv(rc.to_struct(), pcg64_state(e))
        obs0.append(ora.reset().copy())
        oo, rr = [], []
        for t in range(T):
            o, r, dn = ora.step(actions[t, e])
            if dn:
                o = ora.reset()
            oo.append(np.array(o, copy=True))
            rr.append(np.array(r, copy=True))
            done[t, e] = dn
        obs.append(np.stack(oo))
        rew.append(np.stack(rr))
    return dict(actions=actions, obs0=np.stack(obs0), obs=np.stack(obs, 1), rew=np.stack(rew, 1), done=done)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_obs_match_oracle_and_step_x_twin_keeps_the_state(name):
    cfg, _ = CONFIGS[name]
    ref = reference(name)
    try:
        env = VecMaSurvival(cfg, n_envs=N, seeds=range(N), auto_reset=True)
        xen = VecMaSurvival(cfg, n_envs=N, seeds=range(N), auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    assert xen.supports_step_x()
    A, D = env.n_agents, env.obs_dim
    off, shp = env.layout['others_mask']
    assert shp == (A - 1,)
    assert np.array_equal(env.reset().cpu().numpy(), ref['obs0'])
    xen.reset()
    x = torch.zeros((N * A, 8 * ((D + 7) // 8)), dtype=torch.bfloat16, device=xen.device)
    rew = torch.empty((N, A), dtype=torch.float32, device=xen.device)
    dnx = torch.empty((N,), dtype=torch.uint8, device=xen.device)
    deaths = 0
    mask_values = set()
    for t in range(T):
        a = torch.as_tensor(ref['actions'][t], device=env.device)
        o, r, dn, _ = env.step(a)
        xen.step_x(a, x, rew, dnx)
        o = o.cpu().numpy()
        assert np.array_equal(dn.cpu().numpy().astype(bool), ref['done'][t]), (name, t)
        assert np.array_equal(r.cpu().numpy(), ref['rew'][t]), (name, t)
        assert np.array_equal(o, ref['obs'][t]), (name, t)
        assert torch.equal(dn, dnx) and torch.equal(r, rew), (name, t)
        deaths += int((env.alive() == 0).sum())
        mask_values |= set(np.unique(o[..., off:off + A - 1]).tolist())
    assert torch.equal(env.get_state(), xen.get_state()), name
    env.close()
    xen.close()
    print(name, 'dones', int(ref['done'].sum()), 'dead agent-steps', deaths, 'others_mask values', mask_values)
    assert ref['done'].sum() > 0, name  # episodes ended and reset in place
    assert deaths > 0, name  # cameras of dead agents, dead agents as targets
    assert mask_values == {0.0, 1.0}, name
