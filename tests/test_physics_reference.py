"""The physics of the C oracle (oracle/mas_oracle.c) against fp64 closed forms
and invariants (tests/physics_ref.py, tests/physics_laws.py).

The oracle's rules, observations and rewards are pinned by recorded episodes;
its rigid-body step was pinned to nothing but itself, and the HIP kernels are
pinned to the oracle.  Here

  * known answers worked by hand pin every function of the reference itself;
  * the laws of physics_laws.py are applied to oracle episodes driven into
    contact (duels, wall ramming, box seeking) with asserted coverage, so a
    wrong damping form, inverse inertia, TOI target or ray root in the
    restatement fails here (the mutant table is in profiles/physics_laws.txt);
  * ora_sincos is the correctly rounded fp32 of fp64 sin / cos.

MAS_PHYSICS_LAWS_ORACLE=<path to a libmas_oracle.so> runs this module against
another build of the oracle (how the mutants were run); nothing else reads it."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import oracle
import physics_laws as pl
import physics_ref as pr
from masurvival.config import ResolvedConfig, pcg64_state

if os.environ.get('MAS_PHYSICS_LAWS_ORACLE'):
    assert oracle._lib is None, 'the oracle library is already loaded'
    oracle.LIB = os.environ['MAS_PHYSICS_LAWS_ORACLE']

K = 60.0 / 60.8  # 1 / (1 + 0.8 / 60)


# ---------------------------------------------------------------------------
# known answers: the reference itself
# ---------------------------------------------------------------------------
def _rows(C, pos, angle=None, vel=None, omega=None, health=None, boxes=(), heals=(), items=(), removed=()):
    """One env's rows written cell by cell through the layout, then decoded:
    pos [A, 2] ...; boxes: (local verts [4, 2], (x, y), angle); heals, items:
    (x, y); removed: agents whose body is gone (an all-zero row)."""
    A = C.A
    obs = np.zeros((1, A, C.dim), dtype=np.float32)
    lay = C.layout
    pos = np.asarray(pos, dtype=np.float64)
    angle = np.zeros(A) if angle is None else np.asarray(angle, dtype=np.float64)
    vel = np.zeros((A, 2)) if vel is None else np.asarray(vel, dtype=np.float64)
    omega = np.zeros(A) if omega is None else np.asarray(omega, dtype=np.float64)
    health = np.full(A, 100.0) if health is None else np.asarray(health, dtype=np.float64)
    o = lay['agent'][0] + 1 + int(C.rc.has_teams)
    for i in range(A):
        if i not in removed:
            obs[0, i, o:o + 7] = [health[i], pos[i, 0], pos[i, 1], angle[i], vel[i, 0], vel[i, 1], omega[i]]
    for key in ('heals_mask', 'boxes_mask', 'box_items_mask'):
        if key in lay:
            obs[0, :, lay[key][0]:lay[key][0] + lay[key][1][0]] = 1.0
    for b, (verts, p, ang) in enumerate(boxes):
        off = lay['boxes'][0] + 11 * b
        obs[0, :, off:off + 11] = list(np.asarray(verts, dtype=np.float64).reshape(8)) + [p[0], p[1], ang]
        obs[0, :, lay['boxes_mask'][0] + b] = 0.0
    for h, p in enumerate(heals):
        obs[0, :, lay['heals'][0] + 2 * h:lay['heals'][0] + 2 * h + 2] = p
        obs[0, :, lay['heals_mask'][0] + h] = 0.0
    for b, p in enumerate(items):
        obs[0, :, lay['box_items'][0] + 10 * b + 8:lay['box_items'][0] + 10 * b + 10] = p
        obs[0, :, lay['box_items_mask'][0] + b] = 0.0
    return pr.decode(obs, C)


def _acts(*rows):
    return np.array([rows], dtype=np.int8)


BARE_C = pr.constants(pl.BARE)
BOX_C = pr.constants({'melee': pl.MELEE})  # the defaults: 2 agents, 4 heals, 4 boxes
SQUARE = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]
DIAMOND = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
NOOP = (1, 1, 1, 0, 0, 0)


def test_constants_come_from_the_config():
    C = BARE_C
    assert C.r == 0.5 and C.impulse == (0.25, 0.25, 0.0125) and C.floor == 20.0
    assert C.m == pytest.approx(math.pi / 4, rel=1e-15) and C.I == pytest.approx(math.pi / 32, rel=1e-15)
    assert C.k == pytest.approx(K, rel=1e-15) and C.wall_inner == pytest.approx(9.9, rel=1e-15)
    big = pr.constants({'agents': {'n_agents': 2, 'agent_size': 2}, 'motors': {'impulse': (1, 2, 3), 'drift': False},
                        'spawn_grid': {'grid_size': 4, 'floor_size': 30}, 'melee': pl.MELEE})
    assert big.r == 1.0 and big.m == pytest.approx(math.pi) and big.I == pytest.approx(math.pi / 2)
    assert big.impulse == (1.0, 2.0, 3.0) and big.wall_inner == pytest.approx(14.85)
    assert pl.toi_gap(C) == pytest.approx(0.49375, abs=1e-15)


def test_known_answer_push_from_rest():
    """J = 0.25 on m = pi/4: v0 = 1/pi = 0.318310; two world steps damp it to
    v0 k^2 = 0.309989 and move it (1/60) v0 (k + k^2) = 0.01040183.  Agent 1
    faces +y (theta = pi/2) and pushes sideways (left of its nose: -x)."""
    rows = _rows(BARE_C, [(1.0, 2.0), (-3.0, 0.0)], angle=[0.0, math.pi / 2])
    v, w, pos, ang = pr.free_flight(rows, _acts((2, 1, 1, 0, 0, 0), (1, 2, 1, 0, 0, 0)), BARE_C)
    v0 = 1.0 / math.pi
    assert v[0, 0] == pytest.approx([v0 * K * K, 0.0], abs=1e-15)
    assert v[0, 0, 0] == pytest.approx(0.309989, rel=2e-6)
    assert pos[0, 0] == pytest.approx([1.0 + v0 * (K + K * K) / 60.0, 2.0], abs=1e-15)
    assert pos[0, 0, 0] - 1.0 == pytest.approx(0.01040183, rel=2e-6)
    assert v[0, 1] == pytest.approx([-v0 * K * K, 0.0], abs=1e-7)  # pi/2 is an fp32 in the row
    assert pos[0, 1] == pytest.approx([-3.0 - v0 * (K + K * K) / 60.0, 0.0], abs=1e-7)
    assert w[0] == pytest.approx([0.0, 0.0]) and ang[0] == pytest.approx([0.0, math.pi / 2])


def test_known_answer_spin_and_coasting():
    """Jw = 0.0125 on I = pi/32: w0 = 0.4/pi = 0.127324 -> w0 k^2 = 0.123995,
    angle + (1/60) w0 (k + k^2).  A coasting body only damps: (3, -4) k^2."""
    rows = _rows(BARE_C, [(0.0, 0.0), (5.0, 5.0)], vel=[(0.0, 0.0), (3.0, -4.0)], omega=[0.0, 2.0])
    v, w, pos, ang = pr.free_flight(rows, _acts((1, 1, 0, 0, 0, 0), NOOP), BARE_C)
    w0 = 0.4 / math.pi
    assert w[0, 0] == pytest.approx(-w0 * K * K, abs=1e-14) and w[0, 0] == pytest.approx(-0.1239954, rel=2e-6)
    assert ang[0, 0] == pytest.approx(-w0 * (K + K * K) / 60.0, abs=1e-15)
    assert v[0, 1] == pytest.approx([3 * K * K, -4 * K * K], abs=1e-15)
    assert pos[0, 1] == pytest.approx([5 + 3 * (K + K * K) / 60.0, 5 - 4 * (K + K * K) / 60.0], abs=1e-15)
    assert w[0, 1] == pytest.approx(2 * K * K, abs=1e-15)


def test_known_answer_momentum_of_two_bodies():
    """2 m/s meets a body at rest, both pushing forward along +x (J = 0.25
    each): whatever the contact does, sum m v' = k^2 (2 m + 0.5)."""
    C = BARE_C
    prev = _rows(C, [(0.0, 0.0), (1.0, 0.0)], vel=[(2.0, 0.0), (0.0, 0.0)])
    a = _acts((2, 1, 1, 0, 0, 0), (2, 1, 1, 0, 0, 0))
    total = K * K * (2.0 * C.m + 0.5) / C.m
    for v1 in (0.0, 0.3 * total, total):  # any split of the total conserves it
        new = _rows(C, [(0.0, 0.0), (1.0, 0.0)], vel=[(v1, 0.0), (total - v1, 0.0)])
        assert np.abs(pr.momentum_defect(prev, a, new, C)).max() < 1e-6  # the rows are fp32
    # the impulse applied to one body only: the other keeps k^2 (0 + J/m), the defect is the missing share
    new = _rows(C, [(0.0, 0.0), (1.0, 0.0)], vel=[(0.5 * total, 0.0), (K * K * 0.25 / C.m, 0.0)])
    d = pr.momentum_defect(prev, a, new, C)
    assert d[0, 0] == pytest.approx(C.m * (0.5 * total + K * K * 0.25 / C.m - total), abs=1e-6) and abs(d[0, 1]) < 1e-12
    # a dead agent does not count
    new = _rows(C, [(0.0, 0.0), (1.0, 0.0)], vel=[(K * K * (2 + 0.25 / C.m), 0.0), (0.0, 0.0)], health=[100, 0])
    assert np.abs(pr.momentum_defect(prev, a, new, C)).max() < 1e-6


def test_known_answer_gaps_and_pairs():
    C = BOX_C
    s = math.sqrt(0.5)
    rows = _rows(C, [(2.0, 0.0), (1.0, 1.0)], vel=[(0.0, 0.0), (-1.0, -1.0)],
                 boxes=[(SQUARE, (0.0, 0.0), math.pi / 4), (SQUARE, (9.0, -3.0), 0.0)])
    g = pr.box_gaps(rows)
    assert g.shape == (1, 2, 4) and np.isinf(g[0, :, 2:]).all()
    assert g[0, 0, 0] == pytest.approx(2.0 - s, abs=1e-7)               # vertex region: the corner at (0.7071, 0)
    assert g[0, 1, 0] == pytest.approx(math.sqrt(2.0) - 0.5, abs=1e-7)  # face region: the face x + y = 0.7071
    assert g[0, 0, 1] == pytest.approx(math.hypot(6.5, 2.5), abs=1e-7)  # vertex region: the corner at (8.5, -2.5)
    inside = _rows(C, [(0.1, 0.0), (9.2, -3.1)], boxes=[(SQUARE, (0.0, 0.0), math.pi / 4), (SQUARE, (9.0, -3.0), 0.0)])
    gi = pr.box_gaps(inside)
    assert gi[0, 0, 0] == pytest.approx(-(s - 0.1) * s, abs=1e-6) and gi[0, 1, 1] == pytest.approx(-0.3, abs=1e-6)
    # the agents of one row against the boxes of another (a box placed or broken between them)
    bare = _rows(C, [(2.0, 0.0), (1.0, 1.0)])
    assert np.isinf(pr.box_gaps(bare)).all() and np.array_equal(pr.box_gaps(bare, rows), g)
    assert np.isinf(pr.box_gaps(rows, bare)).all()
    w = pr.wall_gaps(_rows(C, [(9.0, -3.0), (0.0, 0.0)], health=[100, 0]), C)
    assert w[0, 0] == pytest.approx([18.9, 12.9, 0.9, 6.9], abs=1e-6) and np.isinf(w[0, 1]).all()
    d = pr.pair_dist(rows)
    assert d[0, 0, 1] == pytest.approx(math.sqrt(2.0)) and d[0, 1, 0] == d[0, 0, 1] and np.isinf(d[0, 0, 0])
    # agent 1 moves at (-1, -1), across the centre line (-1, 1): neither approaching nor separating
    assert pr.pair_normal_speed(rows)[0, 0, 1] == pytest.approx(0.0, abs=1e-12)
    rows = _rows(C, [(0.0, 0.0), (3.0, 4.0)], vel=[(0.0, 0.0), (3.0, 4.0)])
    assert pr.pair_dist(rows)[0, 0, 1] == pytest.approx(5.0) and pr.pair_normal_speed(rows)[0, 0, 1] == pytest.approx(5.0)
    rows = _rows(C, [(0.0, 0.0), (3.0, 4.0)], vel=[(0.6, 0.8), (0.0, 0.0)])
    assert pr.pair_normal_speed(rows)[0, 1, 0] == pytest.approx(-1.0)


def _ray(p1, p2):
    p1, p2 = np.array(p1, dtype=np.float64), np.array(p2, dtype=np.float64)
    return p1, p2 - p1


def test_known_answer_ray_circle():
    on = np.array([True])
    p1, d = _ray((0.0, 0.0), (10.0, 0.0))
    f, g = pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, on)
    assert f[0] == pytest.approx(0.45, abs=1e-15) and not g[0]
    p1, d = _ray((4.8, 0.0), (14.8, 0.0))          # starts inside: no hit
    f, g = pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, on)
    assert np.isinf(f[0]) and not g[0]
    p1, d = _ray((0.0, 0.0), (4.0, 0.0))           # too short
    assert np.isinf(pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, on)[0][0])
    p1, d = _ray((0.0, 0.0), (-10.0, 0.0))         # points away
    assert np.isinf(pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, on)[0][0])
    p1, d = _ray((0.0, 0.50005), (10.0, 0.50005))  # passes 5e-5 above the top: a miss, and grazing
    f, g = pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, on)
    assert np.isinf(f[0]) and g[0]
    p1, d = _ray((0.0, 0.3), (10.0, 0.3))          # off centre: x = 5 - 0.4
    assert pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, on)[0][0] == pytest.approx(0.46, abs=1e-15)
    assert np.isinf(pr.ray_circles(p1, d, np.array([[5.0, 0.0]]), 0.5, np.array([False]))[0][0])


def test_known_answer_ray_polygon():
    on = np.array([True])
    sq = np.array([SQUARE]) + np.array([5.0, 0.0])       # faces at x = 4.5, 5.5, y = -0.5, 0.5
    dia = np.array([DIAMOND]) + np.array([5.0, -1.0])    # its top corner at (5, 0)
    p1, d = _ray((0.0, 0.0), (10.0, 0.0))
    f, g = pr.ray_polygons(p1, d, sq, on)
    assert f[0] == pytest.approx(0.45, abs=1e-15) and not g[0]
    f, g = pr.ray_polygons(p1, d, dia, on)               # grazes the corner: enters and leaves at 0.5
    assert f[0] == pytest.approx(0.5, abs=1e-15) and g[0]
    p1, d = _ray((0.0, 0.001), (10.0, 0.001))            # 1 mm above the corner
    f, g = pr.ray_polygons(p1, d, dia, on)
    assert np.isinf(f[0]) and not g[0]
    p1, d = _ray((0.0, 0.6), (10.0, 0.6))                # parallel to the top face, outside it
    f, g = pr.ray_polygons(p1, d, sq, on)
    assert np.isinf(f[0]) and not g[0]
    p1, d = _ray((5.0, 0.1), (15.0, 0.1))                # starts inside: no entering face
    assert np.isinf(pr.ray_polygons(p1, d, sq, on)[0][0])
    p1, d = _ray((0.0, 0.0), (4.4, 0.0))                 # too short
    assert np.isinf(pr.ray_polygons(p1, d, sq, on)[0][0])
    p1, d = _ray((5.0, 5.0), (5.0, -5.0))                # from above: the face y = 0.5
    assert pr.ray_polygons(p1, d, sq, on)[0][0] == pytest.approx(0.45, abs=1e-15)
    assert np.isinf(pr.ray_polygons(p1, d, sq, np.array([False]))[0][0])


def test_known_answer_lidar_rows():
    """3 lasers over pi, depth 10.  Agent 0 at the origin looks along +x at
    agent 1 (5, 0): the middle ray stops at 4.5, the side rays at the walls'
    inner faces (9.9).  Agent 1's middle ray reaches the right wall at 4.9.
    A heal (r 0.25) at (0, -3) stops agent 0's right-hand ray at 2.75; a box
    at (5, 4) stops agent 1's left-hand ray at 3.5.  A dead agent reads 0."""
    C = pr.constants({'melee': pl.MELEE, 'lidars': {'n_lasers': 3, 'fov': math.pi, 'depth': 10.0}})
    rows = _rows(C, [(0.0, 0.0), (5.0, 0.0)])
    f, g = pr.lidar_ref(rows, C)
    assert f[0] == pytest.approx(np.array([[0.99, 0.45, 0.99], [0.99, 0.49, 0.99]]), abs=1e-12) and not g.any()
    rows = _rows(C, [(0.0, 0.0), (5.0, 0.0)], heals=[(0.0, -3.0)], boxes=[(SQUARE, (5.0, 4.0), 0.0)], items=[(0.0, 6.0)])
    f, g = pr.lidar_ref(rows, C)
    assert f[0] == pytest.approx(np.array([[0.275, 0.45, 0.575], [0.99, 0.49, 0.35]]), abs=1e-12) and not g.any()
    rows = _rows(C, [(0.0, 0.0), (5.0, 0.0)], angle=[math.pi / 2, 0.0], removed=[1])
    f, g = pr.lidar_ref(rows, C)   # turned to +y: the rays go to +x, +y, -x and agent 1 is gone
    assert f[0] == pytest.approx(np.array([[0.99, 0.99, 0.99], [0.0, 0.0, 0.0]]), abs=1e-12)
    # health 0 with a pose: the body is still there for one step, stops rays and casts its own
    rows = _rows(C, [(0.0, 0.0), (5.0, 0.0)], health=[100, 0])
    assert not rows.alive[0, 1] and rows.present[0, 1]
    assert pr.lidar_ref(rows, C)[0][0] == pytest.approx(np.array([[0.99, 0.45, 0.99], [0.99, 0.49, 0.99]]), abs=1e-12)
    assert pr.pair_dist(rows)[0, 0, 1] == 5.0 and np.isinf(pr.wall_gaps(rows, C)[0, 1]).all()
    p1, d = pr.lidar_endpoints(_rows(C, [(0.0, 0.0), (5.0, 0.0)], angle=[math.pi / 2, 0.0]), C)
    assert p1[0, 0] == pytest.approx([0.0, 0.0]) and d[0, 0] == pytest.approx(np.array([[10, 0], [0, 10], [-10, 0]]), abs=1e-6)


def test_known_answer_controllers():
    C = BARE_C
    rows = _rows(C, [(0.0, 0.0), (5.0, -5.0)], angle=[0.0, math.pi / 2])
    a = pr.seek(rows, np.array([[[5.0, -5.0], [5.0, 5.0]]]))
    # agent 0: ahead and to its right; agent 1 faces +y: the target is straight ahead (inside the dead band sideways)
    assert a.dtype == np.int8 and a[0].tolist() == [[2, 0, 2, 0, 0, 0], [2, 1, 2, 0, 0, 0]]
    assert pr.duel(rows)[0].tolist() == [[2, 0, 2, 0, 0, 0], [2, 2, 2, 0, 0, 0]]  # (0, 0) lies ahead-left of agent 1
    dead = _rows(C, [(0.0, 0.0), (5.0, -5.0)], removed=[1])
    assert pr.duel(dead)[0].tolist() == [[1, 1, 2, 0, 0, 0], [1, 1, 1, 0, 0, 0]]  # nobody to seek; the dead do nothing
    C4 = pr.constants(pl.C3_CONFIG)
    rows = _rows(C4, [(0.0, 0.0), (1.0, 0.0), (0.0, -3.0), (9.0, 9.0)], health=[100, 0, 100, 100])
    t = pr.nearest(rows, rows.pos, rows.alive[:, None, :] & ~np.eye(4, dtype=bool)[None])
    assert t[0, 0].tolist() == [0.0, -3.0] and t[0, 3].tolist() == [0.0, 0.0]  # the dead neighbour is skipped
    rows = _rows(BOX_C, [(0.0, 0.0), (8.0, 8.0)], boxes=[(SQUARE, (-4.0, 0.0), 0.0), (SQUARE, (6.0, 6.0), 0.0)])
    assert pr.nearest(rows, rows.box_pos, rows.box_on)[0].tolist() == [[-4.0, 0.0], [6.0, 6.0]]


def test_decode_reads_every_block():
    C = pr.constants(pl.C3_CONFIG)  # teams: the agent block has a team column
    rows = _rows(C, [(1, 2), (3, 4), (5, 6), (7, 8)], angle=[0.1, 0.2, 0.3, 0.4], vel=[(1, 0), (0, 1), (2, 2), (3, 3)],
                 omega=[9, 8, 7, 6], health=[100, 50, 0, 1], removed=[2], boxes=[(SQUARE, (2.0, 3.0), math.pi / 2)],
                 heals=[(4.0, 4.0), (5.0, 5.0)], items=[(6.0, 6.0)])
    assert rows.pos[0].tolist() == [[1, 2], [3, 4], [0, 0], [7, 8]] and rows.alive[0].tolist() == [True, True, False, True]
    assert rows.vel[0, 3].tolist() == [3, 3] and rows.present[0].tolist() == [True, True, False, True] and rows.omega[0].tolist() == [9, 8, 0, 6]
    assert rows.angle[0] == pytest.approx([0.1, 0.2, 0.0, 0.4], abs=1e-7)
    assert rows.heals_on[0].tolist() == [True, True, False, False] and rows.heals[0, 1].tolist() == [5.0, 5.0]
    assert rows.box_on[0].tolist() == [True, False, False, False] and rows.bitems_on[0].tolist() == [True, False, False, False]
    assert rows.bitems[0, 0].tolist() == [6.0, 6.0]
    # the square turned by pi/2 about (2, 3): (-0.5, -0.5) -> (2.5, 2.5)
    assert rows.box_world[0, 0] == pytest.approx(np.array([[2.5, 2.5], [2.5, 3.5], [1.5, 3.5], [1.5, 2.5]]), abs=1e-7)
    walls = pr.wall_polygons(C)
    assert walls[0] == pytest.approx(np.array([[-10.1, -10.0], [-9.9, -10.0], [-9.9, 10.0], [-10.1, 10.0]]), abs=1e-12)
    assert walls[1] == pytest.approx(np.array([[-10.0, 9.9], [10.0, 9.9], [10.0, 10.1], [-10.0, 10.1]]), abs=1e-12)


# ---------------------------------------------------------------------------
# the laws on the oracle
# ---------------------------------------------------------------------------
CPU_SEEDS, CPU_STEPS = 8, 300
LIDAR_SEEDS, LIDAR_STEPS = 6, 80


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """One scenario on the oracle, run once: (Stats, the oracle's counters)."""
    sc = pl.scenario(name)
    n, T = (LIDAR_SEEDS, LIDAR_STEPS) if sc.lidar_only else (CPU_SEEDS, CPU_STEPS)
    rc = ResolvedConfig(sc.cfg)
    envs = [oracle.OracleEnv(rc.to_struct(), pcg64_state(s)) for s in range(n)]

    def step(a):
        out = [e.step(a[k]) for k, e in enumerate(envs)]
        obs = [e.reset() if dn else o for e, (o, _, dn) in zip(envs, out)]
        return np.stack(obs), np.stack([r for _, r, _ in out]), np.array([dn for _, _, dn in out])

    oracle.counters(True)
    st = pl.run(sc, lambda: np.stack([e.reset() for e in envs]), step, range(n), T)
    return sc, st, oracle.counters(True)


@pytest.mark.parametrize('name', pl.SCENARIOS)
def test_oracle_obeys_the_laws(name):
    sc, st, cnt = oracle_run(name)
    print(name, st.report(), {k: v for k, v in cnt.items() if v})
    pl.check(sc, st)
    if name == 'bare_walls':
        assert cnt['toi_event'] > 0
        assert st.worst['min_wall_gap'] >= pl.toi_gap(pr.constants(sc.cfg)) - 1e-5


# ---------------------------------------------------------------------------
# ora_sincos against fp64
# ---------------------------------------------------------------------------
def _sincos_angles():
    rng = np.random.default_rng(7)
    xs = [rng.uniform(-lim, lim, 20000).astype(np.float32) for lim in (4.0, 200.0, 1e4, 1e6)]
    m = (np.arange(-40, 41) * (math.pi / 2)).astype(np.float32)
    xs += [m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf))]
    return np.concatenate(xs)


def test_ora_sincos_is_correctly_rounded_fp64():
    """Every rotation of the step (motors, contacts, rays) goes through
    ora_sincos, and a body's angle is never wrapped, so large arguments are
    real: uniform fp32 angles in +-4, +-200, +-1e4 and +-1e6, and every
    multiple of pi/2 up to +-40 with its fp32 neighbours."""
    L = oracle.lib()
    L.ora_sincos.restype = None
    L.ora_sincos.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    s, c = ctypes.c_float(), ctypes.c_float()
    bad = []
    for x in _sincos_angles().tolist():
        L.ora_sincos(x, ctypes.byref(s), ctypes.byref(c))
        if np.float32(math.sin(x)) != s.value or np.float32(math.cos(x)) != c.value:
            bad.append((x, s.value, c.value))
    assert not bad, (len(bad), bad[:5])
