"""observation.omniscent = False in every capacity class the library builds
(1v1, 2v2, ffa, ffal, xl, xxl), bit for bit against the C oracle.

The non-omniscient camera pass (cameras_v, csrc/mas_post_lanes.h; update_seen
and update_seen_dealt, csrc/mas_step.h) packs (camera << 12) | (lane << 6) |
body into 16 bits, keeps its candidates in a 64-bit mask and sizes its LDS
list per class; it ran on the GPU in one 4-agent config only.  Here each class
runs the config its capacity, facade or lidar test uses, with only the
observation key changed; xxl sits at its full 8 agents, 20 heals and 16 boxes,
64 bodies, so body indices reach 63 and all 8 cameras are live.

64 envs (65 for xxl: a partial last wave) x 120 steps with auto-reset.  The
first half of the steps takes uniform-random actions, the second half the
`hide` or `forage` controller of tests/rules_laws.py, computed from an
omniscient oracle twin, so that cones fill.  Every observation float, reward
and done flag equals the oracle's; each of the four mask blocks the class has
holds both values.  update_seen_dealt runs on the first reset of all envs, on
a masked reset of every third env half way (the other lanes of a block then
only join the dealt rays), and, in the classes whose config has the short
zone (ffal, xxl), on episodes that end and reset in place; under the stock
zone and melee no episode can end within 120 steps.

With the stock camera (fov 0.4 pi, depth 10) a cone covers a tenth of the xxl
room and never holds more than about a quarter of the bodies (the test prints
the most it reached).  The case `xxl_wide` therefore widens the camera of the
same config (fov 0.9 pi, depth 40: nearly the half plane ahead) and asserts,
with rules_ref.cone (the cone test of rules_ref.visible) on the omniscient
twin's rows, that some camera-step
had more than 32 bodies in its cone."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import golden_replay as gr  # noqa: E402
import rules_laws as rl  # noqa: E402
import rules_ref as rr  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival import abi  # noqa: E402
from masurvival.config import C1_CONFIG, C3_CONFIG, C5_CONFIG, ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_capacity import FFA4_BIG, FFA8_BIG  # noqa: E402
from test_gpu_step_x import SIX  # noqa: E402

HI = np.array([3, 3, 3, 2, 2, 2])
T = 120
WIDE = {'fov': 0.9 * np.pi, 'depth': 40}
# class: (config, envs, controller of the second half)
CASES = {
    '1v1': (C1_CONFIG, 64, rl.drive_forage),
    '2v2': (C3_CONFIG, 64, rl.drive_hide),
    'ffa': (C5_CONFIG, 64, rl.drive_hide),
    'ffal': (FFA4_BIG, 64, rl.drive_forage),
    'xl': (SIX, 64, rl.drive_forage),
    'xxl': (FFA8_BIG, 65, rl.drive_hide),
    'xxl_wide': (dict(FFA8_BIG, cameras=WIDE), 64, rl.drive_forage),
}


IN_PLACE = ('ffal', 'xxl', 'xxl_wide')   # configs with the short zone: episodes end within T steps


@functools.lru_cache(maxsize=None)
def reference(name):
    """Oracle twins on the CPU, once per case: the actions [T, N, A, 6], the
    non-omniscient twin's obs0, obs [T, ...], rewards and done flags, and the
    most bodies any camera had in its cone (from the omniscient twin's rows)."""
    cfg, n, driver = CASES[name]
    omni, non = rl.twin_configs(cfg)
    C = rr.constants(cfg)
    tw = [[OracleEnv(ResolvedConfig(c).to_struct(), pcg64_state(s)) for s in range(n)] for c in (omni, non)]
    rng = np.random.default_rng(len(name))
    rows = rr.decode(np.stack([e.reset() for e in tw[0]]), C)
    out = dict(actions=[], obs0=np.stack([e.reset() for e in tw[1]]), obs=[], rew=[], done=[])
    def fill(rows):
        pair, _, cd = rr.cone(rows, C)   # the cone test of rules_ref.visible, without its rays
        return int((pair & (cd <= 0)).sum(-1).max())

    most = fill(rows)
    for t in range(T):
        if t == T // 2:
            obs = res[0][0].copy()
            out['mid'] = np.stack([e.reset() for e in tw[1][::3]])
            obs[::3] = np.stack([e.reset() for e in tw[0][::3]])
            rows = rr.decode(obs, C)
        a = rng.integers(0, HI, size=(n, C.A, 6)).astype(np.int8) if t < T // 2 else driver(t, rows, np.arange(n), rng, C)
        res = []
        for es in tw:
            o = [e.step(a[k]) for k, e in enumerate(es)]
            res.append((np.stack([e.reset() if dn else ob for e, (ob, _, dn) in zip(es, o)]),
                        np.stack([r for _, r, _ in o]), np.array([dn for _, _, dn in o])))
        rows = rr.decode(res[0][0], C)
        most = max(most, fill(rows))
        out['actions'].append(a)
        for key, v in zip(('obs', 'rew', 'done'), res[1]):
            out[key].append(v)
    return {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}, most, C


@pytest.mark.parametrize('name', list(CASES))
def test_nonomniscient_class_matches_oracle(name):
    cfg, n, _ = CASES[name]
    ref, most, C = reference(name)
    non = rl.twin_configs(cfg)[1]
    assert not ResolvedConfig(non).to_struct().omniscient
    try:
        env = VecMaSurvival(non, n_envs=n, seeds=range(n), auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    assert np.array_equal(env.reset().cpu().numpy(), ref['obs0']), name
    third = torch.zeros(n, dtype=torch.uint8)
    third[::3] = 1
    for t in range(T):
        if t == T // 2:
            assert np.array_equal(env.reset(third.to(env.device)).cpu().numpy()[::3], ref['mid']), name
        o, r, dn, _ = env.step(torch.as_tensor(ref['actions'][t], device=env.device))
        o = o.cpu().numpy()
        assert np.array_equal(dn.cpu().numpy().astype(bool), ref['done'][t]), (name, t)
        assert np.array_equal(r.cpu().numpy(), ref['rew'][t]), (name, t)
        if not np.array_equal(o, ref['obs'][t]):
            e = int(np.nonzero((o != ref['obs'][t]).any((1, 2)))[0][0])
            raise AssertionError((name, t, e, gr.diff(o[e], ref['obs'][t][e])))
    guards, invalid = env.debug_guards(), env.invalid_actions()
    env.close()
    assert guards['list_overflow'] == 0 and invalid == 0, (guards, invalid)
    values = {}
    for key in rr.MASK_KEYS:
        if key in C.layout:
            off, shp = C.layout[key]
            values[key] = set(np.unique(ref['obs'][..., off:off + shp[0]]).tolist())
    print(name, 'resets', int(ref['done'].sum()), 'most bodies in a cone', most, 'of', C.M - 1, values)
    if name in IN_PLACE:
        assert ref['done'].sum() > 0, name                # update_seen_dealt ran on in-place resets
    assert all(v == {0.0, 1.0} for v in values.values()) and len(values) == (4 if C.B and C.H else 1), (name, values)
    if name == 'xxl_wide':
        assert C.M + 4 == 64 and most > 32, most   # 60 bodies with a mask and the four walls
