"""The rules' geometry of the C oracle (oracle/mas_oracle.c) against an fp64
reference written from the geometry (tests/rules_ref.py, tests/rules_laws.py):
who sees whom, whom a swing hits, which item is picked up, who stands outside
the zone.

The recorded episodes pin these only to the reference's Python running over
ray casts and point tests that are the oracle's own, and the HIP kernels are
pinned to the oracle.  Here

  * known answers worked by hand pin every function of rules_ref itself;
  * the laws of rules_laws.py are applied to oracle twins (the same config,
    seeds and actions with observation.omniscent True and False) driven to
    hide, forage, brawl and walk the zone's rim, with asserted coverage, so a
    wrong cone, first hit, reach or radius test in the oracle fails here (the
    mutant table is in profiles/rules_laws.txt).

MAS_PHYSICS_LAWS_ORACLE=<path to a libmas_oracle.so>, read by
test_physics_reference, runs this module too against another build of the
oracle (how the mutants were run)."""
import functools
import math

import numpy as np
import pytest

import oracle
import rules_laws as rl
import rules_ref as rr
from masurvival.config import ResolvedConfig, pcg64_state
from physics_laws import MELEE
from test_physics_reference import SQUARE, _rows

C4 = rr.constants({'agents': {'n_agents': 4, 'agent_size': 1}, 'melee': MELEE})  # 4 agents, 4 heals, 4 boxes
HALF = 0.2 * math.pi   # half of the stock fov, 36 degrees
CAM = (-5.0, 0.0)      # the camera of the known answers: agent 0, looking along +x
SLAT = [(-0.1, -1.0), (0.1, -1.0), (0.1, 1.0), (-0.1, 1.0)]
GONE = [2, 3]


def _polar(r, a):
    return (CAM[0] + r * math.cos(a), CAM[1] + r * math.sin(a))


def _see(target, **kw):
    """visible() of agent 1 at `target` from the camera"""
    rows = _rows(C4, [CAM, target, (0, 0), (0, 0)], removed=GONE, **kw)
    V = rr.visible(rows, C4)
    return bool(V.in_cone[0, 0, 1]), bool(V.first[0, 0, 1]), bool(V.graze[0, 0, 1])


# ---------------------------------------------------------------------------
# known answers: the reference itself
# ---------------------------------------------------------------------------
def test_constants_and_cone_polygon():
    C = C4
    assert (C.A, C.H, C.B, C.M) == (4, 4, 4, 16) and C.fov == pytest.approx(0.4 * math.pi) and C.depth == 10.0
    assert (C.melee_range, C.damage, C.cooldown, C.healing, C.slots) == (2.0, 20, 40, 50, 4)
    assert (C.pickup_r, C.zone_damage, C.box_health) == (0.5, 1, 20)
    assert rr.constants({'melee': {'range': 3, 'damage': 5, 'drift': True}}).cooldown == 0   # continuous melee
    assert C.kind.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 and C.index[4:8].tolist() == [0, 1, 2, 3]
    # 10 (cos 36, sin 36) = (8.0902, 5.8779)
    assert rr.cone_polygon(C) == pytest.approx(np.array([[0, 0], [8.0902, -5.8779], [10, 0], [8.0902, 5.8779]]), abs=1e-4)


def test_known_answer_cone_axis_and_depth():
    """On the axis the cone ends at the depth vertex, 10 m from the camera."""
    assert _see(_polar(10.0 - 1e-3, 0.0)) == (True, True, False)
    assert _see(_polar(10.0 + 1e-3, 0.0)) == (False, False, False)
    assert _see(_polar(10.0 - 5e-5, 0.0))[::2] == (True, True) and _see(_polar(10.0 + 5e-5, 0.0))[::2] == (False, True)
    # beyond the chord between the two far corners (x = 8.09) the depth vertex still counts
    assert _see(_polar(9.0, 0.0)) == (True, True, False)
    assert _see(_polar(1.5, math.pi)) == (False, False, False)   # behind the camera


def test_known_answer_cone_slanted_edges():
    """The edges from the apex run at +-36 degrees: at 4 m, 1 mm of arc is
    2.5e-4 rad.  The edges to the depth vertex are chords of the 10 m circle
    between 0 and +-36 degrees: their midpoints lie 10 cos 18 = 9.5106 m out at
    +-18 degrees, with the outward normal along that bearing."""
    for sign in (1.0, -1.0):
        assert _see(_polar(4.0, sign * (HALF - 2.5e-4))) == (True, True, False)
        assert _see(_polar(4.0, sign * (HALF + 2.5e-4))) == (False, False, False)
        assert _see(_polar(4.0, sign * (HALF - 1e-5)))[2] and _see(_polar(4.0, sign * (HALF + 1e-5)))[2]
        mid = 10.0 * math.cos(HALF / 2.0)
        assert mid == pytest.approx(9.5106, abs=1e-4)
        assert _see(_polar(mid - 1e-3, sign * HALF / 2.0)) == (True, True, False)
        assert _see(_polar(mid + 1e-3, sign * HALF / 2.0)) == (False, False, False)
        # half the fov is the half angle: 50 degrees off the axis is outside, 30 inside
        assert not _see(_polar(4.0, sign * math.radians(50)))[0] and _see(_polar(4.0, sign * math.radians(30)))[0]
    # the cone turns with the camera: facing +y, a body straight above is seen, one along +x is not
    rows = _rows(C4, [CAM, (-5.0, 4.0), (-1.0, 0.0), (0, 0)], angle=[math.pi / 2, 0, 0, 0], removed=[3])
    V = rr.visible(rows, C4)
    assert V.seen[0, 0, 1] and not V.in_cone[0, 0, 2] and not V.pair[0, 0, 0] and not V.pair[0, 0, 3]


def test_known_answer_heal_behind_a_box_and_behind_an_agent():
    """A slat 0.2 x 2 at (-2, 0.8) spans y in [-0.8, 1.8] across the axis and
    hides the heal at (1, 0); turned by pi/2 it spans y in [0.7, 0.9] and the
    heal shows.  The box itself is seen either way (its centre is 18 degrees
    up)."""
    h, b = C4.A, C4.A + C4.H
    rows = _rows(C4, [CAM, (0, 0), (0, 0), (0, 0)], removed=[1, 2, 3], heals=[(1.0, 0.0)], boxes=[(SLAT, (-2.0, 0.8), 0.0)])
    V = rr.visible(rows, C4)
    assert V.in_cone[0, 0, h] and not V.first[0, 0, h] and not V.seen[0, 0, h] and V.occluder[0, 0, h] == rr.BOX
    assert V.seen[0, 0, b] and not V.graze[0, 0, h] and not V.graze[0, 0, b]
    rows = _rows(C4, [CAM, (0, 0), (0, 0), (0, 0)], removed=[1, 2, 3], heals=[(1.0, 0.0)], boxes=[(SLAT, (-2.0, 0.8), math.pi / 2)])
    V = rr.visible(rows, C4)
    assert V.seen[0, 0, h] and V.occluder[0, 0, h] == rr.NONE and V.seen[0, 0, b]
    assert not V.pair[0, 0, h + 1] and not V.seen[0, 0, h + 1]          # an empty slot is nobody
    # the slat's corner 5e-5 above the line of sight: a miss, and grazing
    rows = _rows(C4, [CAM, (0, 0), (0, 0), (0, 0)], removed=[1, 2, 3], heals=[(1.0, 0.0)], boxes=[(SLAT, (-2.0, 1.00005), 0.0)])
    V = rr.visible(rows, C4)
    assert V.seen[0, 0, h] and V.graze[0, 0, h]
    # agents in a row: the nearer one is seen and hides the farther; a heal (a sensor) hides too
    rows = _rows(C4, [CAM, (-2.0, 0.0), (1.0, 0.0), (0, 0)], removed=[3], heals=[(3.0, 3.0)])
    V = rr.visible(rows, C4)
    assert V.seen[0, 0, 1] and V.in_cone[0, 0, 2] and not V.seen[0, 0, 2] and V.occluder[0, 0, 2] == rr.AGENT
    assert V.seen[0, 0, h]
    rows = _rows(C4, [CAM, (1.0, 0.0), (0, 0), (0, 0)], removed=GONE, heals=[(-2.0, 0.1)])
    V = rr.visible(rows, C4)
    assert not V.seen[0, 0, 1] and V.occluder[0, 0, 1] == rr.HEAL and V.seen[0, 0, h]
    # agent 1 looks along +x too: the camera is behind it
    assert not V.in_cone[0, 1, 0] and not V.seen[0, 1, 0]
    # a removed camera sees nothing, and nobody sees it
    assert not V.pair[0, 2].any() and not V.pair[0, :, 2].any()


def test_known_answer_camera_inside_a_heal():
    """The heal's circle (r 0.25) at 0.1 m ahead holds the camera's centre:
    the line of sight starts inside it and hits nothing."""
    h = C4.A
    rows = _rows(C4, [CAM, (0, 0), (0, 0), (0, 0)], removed=[1, 2, 3], heals=[(-4.9, 0.0)])
    V = rr.visible(rows, C4)
    assert V.in_cone[0, 0, h] and not V.first[0, 0, h] and not V.seen[0, 0, h] and V.occluder[0, 0, h] == rr.NONE
    rows = _rows(C4, [CAM, (0, 0), (0, 0), (0, 0)], removed=[1, 2, 3], heals=[(-4.7, 0.0)])   # 0.3 m: outside it
    assert rr.visible(rows, C4).seen[0, 0, h]
    rows = _rows(C4, [CAM, (0, 0), (0, 0), (0, 0)], removed=[1, 2, 3], heals=[(-4.75003, 0.0)])  # on its skin
    assert rr.visible(rows, C4).graze[0, 0, h]


def test_known_answer_melee_target():
    """Range 2 from the centre along the heading.  A heal at 1 m (skin at 0.75)
    stands before the agent at 1.4 m (skin at 0.9)."""
    rows = _rows(C4, [CAM, (-3.6, 0.0), (0, 0), (0, 0)], removed=GONE, heals=[(-4.0, 0.0)])
    T = rr.melee_target(rows, C4)
    assert (T.kind[0, 0], T.idx[0, 0]) == (rr.HEAL, 0) and not T.graze[0, 0] and T.reach[0, 0].tolist() == [False, True, False, False]
    assert T.kind[0, 1] == rr.NONE and T.kind[0, 2] == rr.NONE     # agent 1 swings at nothing; agent 2 is gone
    rows = _rows(C4, [CAM, (-3.6, 0.0), (0, 0), (0, 0)], removed=GONE)
    T = rr.melee_target(rows, C4)
    assert (T.kind[0, 0], T.idx[0, 0]) == (rr.AGENT, 1)
    # the range counts from the swinger's centre: a skin at 1.9 m is hit, one at 2.1 m is not
    assert rr.melee_target(_rows(C4, [CAM, (-2.6, 0.0), (0, 0), (0, 0)], removed=GONE), C4).kind[0, 0] == rr.AGENT
    assert rr.melee_target(_rows(C4, [CAM, (-2.4, 0.0), (0, 0), (0, 0)], removed=GONE), C4).kind[0, 0] == rr.NONE
    T = rr.melee_target(_rows(C4, [CAM, (-2.50005, 0.0), (0, 0), (0, 0)], removed=GONE), C4)
    assert T.kind[0, 0] == rr.AGENT and T.graze[0, 0]
    # a box, a box item and a wall; the heading turns the swing
    rows = _rows(C4, [CAM, (-5.0, 1.2), (-9.0, 0.0), (0, 0)], angle=[0, math.pi / 2, math.pi, 0], removed=[3],
                 boxes=[(SQUARE, (-3.5, 0.0), 0.0)], items=[(-5.0, 2.5)])
    T = rr.melee_target(rows, C4)
    assert [(int(k), int(i)) for k, i in zip(T.kind[0], T.idx[0])] == [(rr.BOX, 0), (rr.BITEM, 0), (rr.WALL, 0), (rr.NONE, -1)]
    # an agent off the line by more than its radius is out of reach
    rows = _rows(C4, [CAM, (-4.0, 0.6), (0, 0), (0, 0)], removed=GONE)
    T = rr.melee_target(rows, C4)
    assert T.kind[0, 0] == rr.NONE and not T.reach[0, 0].any() and not T.graze[0, 0]


def test_known_answer_in_radius():
    inside, graze = rr.in_radius([(3.0, 4.0), (3.0, 4.0), (0.3, 0.4), (0.30003, 0.4)], [(0.0, 0.0)] * 4,
                                 np.array([5.1, 4.9, 0.5, 0.5]))
    assert inside.tolist() == [True, False, True, False] and graze.tolist() == [False, False, True, True]
    inside, graze = rr.in_radius(np.zeros((2, 3, 2)), np.ones((2, 1, 2)), 1.5)
    assert inside.shape == (2, 3) and inside.all() and not graze.any()
    assert not rr.in_radius([(0.0, 1e-3)], [(0.0, 0.0)], 0.0)[0][0]   # the endgame's zone: everybody is outside


def test_decode_and_masks_read_every_block():
    C = rr.constants(rl.scenario('brawl_2v2').cfg)       # teams: a team column
    obs = np.zeros((1, C.A, C.dim), dtype=np.float32)
    lay = C.layout
    for key in rr.MASK_KEYS + ('heal_slot_mask', 'box_slot_mask'):
        obs[0, :, lay[key][0]:lay[key][0] + int(np.prod(lay[key][1]))] = 1.0
    obs[0, :, lay['agent'][0] + 1] = [0, 0, 1, 1]
    obs[0, :, lay['agent'][0] + 2] = 100.0
    obs[0, :, lay['zone'][0]:lay['zone'][0] + 6] = [1, 2, 3, 4, 5, 6]
    obs[0, 2, lay['others_mask'][0] + 2] = 0.0           # agent 2's third other is agent 3
    obs[0, 0, lay['others_mask'][0] + 0] = 0.0           # agent 0's first other is agent 1
    obs[0, 1, lay['heals_mask'][0] + 3] = 0.0
    obs[0, 3, lay['boxes_mask'][0] + 1] = 0.0
    obs[0, 3, lay['box_items_mask'][0] + 2] = 0.0
    obs[0, 1, lay['heal_slot_mask'][0]] = 0.0
    obs[0, 2, lay['box_slot_mask'][0]] = 0.0
    R = rr.decode(obs, C)
    assert R.team[0].tolist() == [0, 0, 1, 1] and R.zone[0].tolist() == [1, 2, 3, 4, 5, 6]
    assert R.heal_slot[0].tolist() == [False, True, False, False] and R.box_slot[0].tolist() == [False, False, True, False]
    seen, raw = rr.masks(obs, C)
    want = np.zeros((C.A, C.M), dtype=bool)
    want[2, 3] = want[0, 1] = want[1, C.A + 3] = want[3, C.A + C.H + 1] = want[3, C.A + C.H + C.B + 2] = True
    assert np.array_equal(seen[0], want) and set(raw) == set(rr.MASK_KEYS)
    cols = rr.mask_columns(C)
    assert cols.sum() == (C.A - 1) + C.H + 2 * C.B and cols[lay['boxes_mask'][0]] and not cols[lay['heal_slot_mask'][0]]
    assert rr.decode(np.zeros((1, 2, rr.constants({'melee': MELEE}).dim), dtype=np.float32), rr.constants({'melee': MELEE})).team[0].tolist() == [0, 1]


# ---------------------------------------------------------------------------
# the laws on the oracle
# ---------------------------------------------------------------------------
CPU_SEEDS, CPU_STEPS = 8, 300


def oracle_twins(cfg, seeds):
    """(reset, step) of rules_laws.run over two lists of oracle envs."""
    envs = [[oracle.OracleEnv(ResolvedConfig(c).to_struct(), pcg64_state(s)) for s in seeds] for c in rl.twin_configs(cfg)]

    def reset():
        return tuple(np.stack([e.reset() for e in es]) for es in envs)

    def step(a):
        res = []
        for es in envs:
            out = [e.step(a[k]) for k, e in enumerate(es)]
            obs = [e.reset() if dn else o for e, (o, _, dn) in zip(es, out)]
            res.append((np.stack(obs), np.stack([r for _, r, _ in out]), np.array([dn for _, _, dn in out])))
        return res

    return reset, step


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    sc = rl.scenario(name)
    reset, step = oracle_twins(sc.cfg, range(CPU_SEEDS))
    return sc, rl.run(sc, reset, step, range(CPU_SEEDS), CPU_STEPS)


@pytest.mark.parametrize('name', rl.SCENARIOS)
def test_oracle_obeys_the_laws(name):
    sc, st = oracle_run(name)
    print(name, st.report())
    rl.check(sc, st)


def test_scenarios_cover_both_melee_forms():
    forms = {rr.constants(rl.scenario(n).cfg).cooldown for n in rl.SCENARIOS if n.startswith('brawl')}
    assert forms == {0, 40}
