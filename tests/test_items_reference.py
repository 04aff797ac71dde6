"""Where items go in the C oracle (oracle/mas_oracle.c) against an fp64 item
ledger written from the reference's text (tests/items_ref.py,
tests/items_laws.py): the world a reset deals, placing a box, give, the tops of
the inventories, conservation, death drops and box ownership.

The recorded episodes pin these only to the reference's Python running over
queries, rotations and polygons that are the oracle's own, and the HIP kernels
are pinned to the oracle.  Here

  * known answers worked by hand pin every function of items_ref and the
    ledger itself (the copy on a double pickup, the item lost to a full taker,
    a placed box, a spawn refused for want of a slot, a stack dropped at the
    radius, a box only its owner breaks);
  * the laws of items_laws.py are applied to the oracle driven to hand items
    over, to build and to loot, with asserted coverage, so a wrong taker,
    placement, drop or owner in the oracle fails here (the mutant table is in
    profiles/items_laws.txt).

MAS_PHYSICS_LAWS_ORACLE=<path to a libmas_oracle.so>, read by
test_physics_reference, runs this module too against another build of the
oracle (how the mutants were run)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import items_laws as il
import items_ref as ir
import oracle
import rules_laws as rl
import rules_ref as rr
from masurvival.config import ResolvedConfig, pcg64_state
from physics_laws import MELEE, Stats
from test_physics_reference import K, SQUARE, _rows

C4 = ir.constants({'agents': {'n_agents': 4, 'agent_size': 1}, 'melee': MELEE})   # 4 agents, 4 heals, 4 boxes, 4 slots
C4_1 = ir.constants({'agents': {'n_agents': 4, 'agent_size': 1}, 'melee': MELEE, 'inventory': {'slots': 1}})
FAR = [(-8.0, -8.0), (8.0, -8.0), (8.0, 8.0), (-8.0, 8.0)]    # four agents out of each other's way
SLAT = [(-0.1, -1.0), (0.1, -1.0), (0.1, 1.0), (-0.1, 1.0)]   # 0.2 x 2 in SetAsBox order


def _f32bits(v):
    return tuple(int(x) for x in np.asarray(v, dtype=np.float32).reshape(-1).view(np.uint32))


# ---------------------------------------------------------------------------
# known answers: the reference itself
# ---------------------------------------------------------------------------
def test_constants_come_from_the_config():
    C = C4
    assert (C.give_r, C.drop_r, C.offset, C.grid, C.box_size) == (2.0, 0.5, 0.75, 4, 1.0)
    assert (C.randomized, C.ownership, C.full_health, C.zone_r0, C.slots) == (False, False, 100, 10.0, 4)
    D = ir.constants(il.scenario('builder').cfg)
    assert D.randomized and D.ownership and (D.min_w, D.min_h, D.grid) == (0.1, 0.1, 8)
    assert ir.constants(il.scenario('loot').cfg).drop_r == 1.0
    assert ir.wall_centres(C).tolist() == [[-10, 0], [0, 10], [10, 0], [0, -10]]


def _taker(pos, removed=(2, 3), extra=None, **kw):
    rows = _rows(C4, pos, removed=removed, **kw)
    T = ir.give_taker(rows, C4, extra)
    return (int(T.kind[0, 0]), int(T.idx[0, 0]), bool(T.graze[0, 0])), T


def test_known_answer_give_radius():
    """The give circle has radius 2 about the giver's centre and takes the
    other's centre, not its skin."""
    assert _taker([(0, 0), (1.9999, 0), (0, 0), (0, 0)])[0][:2] == (rr.AGENT, 1)
    assert _taker([(0, 0), (2.0001, 0), (0, 0), (0, 0)])[0][:2] == (rr.NONE, -1)
    assert _taker([(0, 0), (1.99995, 0), (0, 0), (0, 0)])[0] == (rr.AGENT, 1, True)
    assert _taker([(0, 0), (2.00005, 0), (0, 0), (0, 0)])[0] == (rr.NONE, -1, True)
    assert _taker([(0, 0), (1.5, 0), (0, 0), (0, 0)])[0] == (rr.AGENT, 1, False)
    # a skin within 2 m is not enough: centre at 2.4, skin at 1.9
    assert _taker([(0, 0), (2.4, 0), (0, 0), (0, 0)])[0] == (rr.NONE, -1, False)
    # the circle moves with the giver and ignores its heading
    assert _taker([(3, 4), (3, 5.9), (0, 0), (0, 0)], angle=[2.0, 0, 0, 0])[0] == (rr.AGENT, 1, False)
    # a removed agent gives to nobody and is nobody's taker; an agent is not its own
    (k, i, g), T = _taker([(0, 0), (1.0, 0), (0, 0), (0.5, 0)])
    assert (k, i) == (rr.AGENT, 1) and T.kind[0, 2] == rr.NONE and T.kind[0, 3] == rr.NONE
    assert T.kind[0, 1] == rr.AGENT and T.idx[0, 1] == 0 and T.reach[0, 0].tolist() == [False, True, False, False]


def test_known_answer_give_takes_the_nearest_body_of_any_kind():
    """A heal at 0.8 m is nearer than an agent at 1.2 m; so is a box at 1 m, a
    box item, a wall's centre, a box placed in this step."""
    pos = [(0, 0), (1.2, 0), (0, 0), (0, 0)]
    assert _taker(pos, heals=[(0, 0.8)])[0] == (rr.HEAL, 0, False)
    assert _taker(pos, heals=[(5, 5), (0, -1.5)])[0] == (rr.AGENT, 1, False)
    assert _taker(pos, boxes=[(SQUARE, (-1.0, 0), 0.0)])[0] == (rr.BOX, 0, False)
    assert _taker(pos, items=[(5, 5), (0.6, 0.6)])[0] == (rr.BITEM, 1, False)
    # not the first in range: the farther body comes first in every list
    assert _taker([(0, 0), (1.9, 0), (0, 1.0), (0, 0)], removed=[3])[0] == (rr.AGENT, 2, False)
    # two candidates 5e-5 apart in distance
    assert _taker(pos, heals=[(0, 1.20005)])[0][2] and not _taker(pos, heals=[(0, 1.2005)])[0][2]
    # the right wall's centre is at (10, 0): 1.5 m from (8.5, 0)
    assert _taker([(8.5, 0), (0, 0), (0, 0), (0, 0)])[0] == (rr.WALL, 2, False)
    assert _taker([(8.5, 1.0), (8.5, 2.5), (0, 0), (0, 0)])[0] == (rr.AGENT, 1, False)     # wall centre at 1.80, agent at 1.5
    assert _taker([(8.5, 1.5), (0, 0), (0, 0), (0, 0)])[0] == (rr.NONE, -1, False)         # 2.12 m: the wall's skin is nearer
    # a box placed by agent 1 in this step, 0.75 m ahead of agent 0's neighbour
    X = SimpleNamespace(pos=np.array([[(0.0, 0.0), (0.7, 0.0)]]), on=np.array([[False, True]]),
                        kind=np.full((1, 2), ir.PLACED), idx=np.array([[0, 1]]))
    assert _taker(pos, extra=X)[0] == (ir.PLACED, 1, False)
    X.on[0, 1] = False
    assert _taker(pos, extra=X)[0] == (rr.AGENT, 1, False)


def test_known_answer_placement():
    p = np.array([1.0, 2.0])
    for ang, want in ((0.0, (1.75, 2.0)), (math.pi / 2, (1.0, 2.75)), (math.pi, (0.25, 2.0)), (-math.pi / 2, (1.0, 1.25))):
        assert ir.placement(p, ang, 0.75) == pytest.approx(want, abs=1e-15)
    out = ir.placement(np.zeros((2, 3, 2)), np.full((2, 3), math.pi / 6), 2.0)
    assert out.shape == (2, 3, 2) and out[1, 2] == pytest.approx((math.sqrt(3), 1.0))


def test_known_answer_spawn_cells():
    cells = ir.spawn_cells(C4)                      # grid 4, floor 20: centres at -7.5, -2.5, 2.5, 7.5
    assert cells.shape == (16, 2)
    assert cells[0].tolist() == [-7.5, -7.5] and cells[1].tolist() == [-2.5, -7.5] and cells[4].tolist() == [-7.5, -2.5]
    assert cells[15].tolist() == [7.5, 7.5] and sorted(set(cells[:, 0].tolist())) == [-7.5, -2.5, 2.5, 7.5]
    big = ir.spawn_cells(ir.constants(il.scenario('loot').cfg))      # grid 8: 2.5 m cells
    assert big.shape == (64, 2) and big[0].tolist() == [-8.75, -8.75] and big[9].tolist() == [-6.25, -6.25]


def test_known_answer_rect_dims_and_item_shape():
    w, h, ok = ir.rect_dims(np.array(SLAT))
    assert (w, h, bool(ok)) == (pytest.approx(0.2), pytest.approx(2.0), True)
    swapped = [SLAT[1], SLAT[0], SLAT[2], SLAT[3]]
    assert not ir.rect_dims(np.array(swapped))[2]
    assert not ir.rect_dims(np.array(SLAT) + 0.01)[2]                                # off centre
    assert not ir.rect_dims(np.array(SLAT)[[1, 2, 3, 0]])[2]                         # the same loop started elsewhere
    w, h, ok = ir.rect_dims(np.array([SLAT, SQUARE]))
    assert w.tolist() == pytest.approx([0.2, 1.0]) and ok.tolist() == [True, True]
    # the item's loop starts at the rightmost vertex, the lower of the two: (w/2, -h/2)
    item = ir.item_shape(_f32bits(SLAT))
    assert item == _f32bits([SLAT[1], SLAT[2], SLAT[3], SLAT[0]]) and ir.item_shape(item) == item


def test_known_answer_corpse_and_max_step():
    """Forward thrust from rest: v = J / m, x' = x + H v (k + k^2)."""
    C = C4
    rows = _rows(C, [(0, 0), (9.3, 0.0), (3.0, 3.0), (3.9, 3.0)], vel=[(0, 0), (0, 0), (0, 0), (0, 0)])
    acts = np.array([[(2, 1, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0)]], dtype=np.int8)
    pos, free = ir.corpse(rows, C, acts)
    v = 0.25 / (math.pi / 4)
    assert pos[0, 0] == pytest.approx((v * (K + K * K) / 60.0, 0.0), rel=1e-12)
    assert free[0].tolist() == [True, False, False, False]          # next to a wall; a touching pair
    assert ir.max_step(rows, C, acts)[0] == pytest.approx(2 * (v / 60.0 + 0.2))
    rows = _rows(C, FAR, boxes=[(SQUARE, (-8.0, -7.0), 0.0)], removed=[3])
    assert ir.corpse(rows, C, acts)[1][0].tolist() == [False, True, True, False]   # at a box; removed


# ---------------------------------------------------------------------------
# known answers: the ledger
# ---------------------------------------------------------------------------
def _world(C, pos, tops=(), item_shapes=(), **kw):
    """_rows plus what items_ref.decode adds: tops[i] is None, 'heal' or a
    vertex loop; item_shapes the loops of the box items on the ground."""
    R = _rows(C, pos, **kw)
    A = C.A
    R.team = np.broadcast_to(np.arange(A), (1, A))
    R.zone = np.array([[0.0, 0.0, 10.0, 0.0, 0.0, 5.0]])
    R.box_bits = np.ascontiguousarray(R.box_local.reshape(1, -1, 8).astype(np.float32)).view(np.uint32)
    R.box_item_bits = ir.item_shapes(R.box_bits)
    R.bitem_bits = np.zeros((1, C.B, 8), dtype=np.uint32)
    for k, s in enumerate(item_shapes):
        R.bitem_bits[0, k] = _f32bits(s)
    R.top_bits, R.heal_amount, R.slot_raw = np.zeros((1, A, 8), dtype=np.uint32), np.zeros((1, A)), np.ones((1, A, 2))
    for i, top in enumerate(tuple(tops) + (None,) * (A - len(tops))):
        if isinstance(top, str):
            R.heal_amount[0, i], R.slot_raw[0, i, 0] = C.healing, 0.0
        elif top is not None:
            R.top_bits[0, i], R.slot_raw[0, i, 1] = _f32bits(top), 0.0
    R.heal_slot, R.box_slot = R.slot_raw[..., 0] == 0, R.slot_raw[..., 1] == 0
    return R


def _play(C, prev, new, actions, stacks, owners=None):
    """One step of the laws on hand-made rows, from the given stacks."""
    L, st = il.Ledger(1, C), Stats()
    L.reset(np.ones(1, dtype=bool), prev)
    for i, s in enumerate(stacks):
        L.stack[0][i] = list(s)
    L.owner[0].update(owners or {})
    a = np.array([actions], dtype=np.int8)
    valid = np.ones(1, dtype=bool)
    led = rl.law_ledger(C, prev, new, a, valid, L.rules, Stats(), 0)
    il.law_items(C, prev, new, a, valid, led, L, st, 0)
    il.law_tops(C, new, L, valid, st, 0)
    return L, st.count, st


NOOP, USE, GIVE = (1, 1, 1, 0, 0, 0), (1, 1, 1, 0, 1, 0), (1, 1, 1, 0, 0, 1)
HEAL = il.HEAL_ITEM


def test_ledger_copies_an_item_two_agents_reach_together():
    """A heal between two agents, 0.45 m from each: both take it, the heal is
    gone once and held twice."""
    pos = [(-0.45, 0.0), (0.45, 0.0), FAR[2], FAR[3]]
    prev = _world(C4, pos, heals=[(0.0, 0.0), (5.0, 5.0)])
    new = _world(C4, pos, heals=[(5.0, 5.0)], tops=('heal', 'heal'))
    L, c, _ = _play(C4, prev, new, [NOOP] * 4, [[], [], [], []])
    assert L.stack[0][0] == [HEAL] and L.stack[0][1] == [HEAL] and c['double_pickups'] == 1 and c['pickups'] == 1
    assert c.get('top_wrong', 0) == 0 and c.get('conserve_wrong', 0) == 0 and c['conserve_steps'] == 1
    # the row of an engine that gives it to the first agent alone
    new = _world(C4, pos, heals=[(5.0, 5.0)], tops=('heal', None))
    assert _play(C4, prev, new, [NOOP] * 4, [[], [], [], []])[1]['top_wrong'] == 1
    # a full agent takes nothing: one slot, already filled
    new = _world(C4_1, pos, heals=[(5.0, 5.0)], tops=('heal', 'heal'))
    L, c, _ = _play(C4_1, prev, new, [NOOP] * 4, [[HEAL], []])
    assert c.get('double_pickups', 0) == 0 and c.get('top_wrong', 0) == 0 and c.get('conserve_wrong', 0) == 0


def test_ledger_loses_the_item_given_to_a_full_taker():
    """One slot each, both hold a heal, agent 0 gives: its heal is popped and
    agent 1 cannot take it."""
    pos = [(0.0, 0.0), (1.2, 0.0), FAR[2], FAR[3]]
    prev = _world(C4_1, pos, tops=('heal', 'heal'))
    new = _world(C4_1, pos, tops=(None, 'heal'))
    L, c, _ = _play(C4_1, prev, new, [GIVE, NOOP, NOOP, NOOP], [[HEAL], [HEAL]])
    assert L.stack[0][0] == [] and L.stack[0][1] == [HEAL] and c['give_lost'] == 1
    assert c.get('top_wrong', 0) == 0 and c.get('conserve_wrong', 0) == 0 and c['conserve_steps'] == 1
    # the row of an engine that leaves the item with the giver
    assert _play(C4_1, prev, prev, [GIVE, NOOP, NOOP, NOOP], [[HEAL], [HEAL]])[1]['top_wrong'] == 1
    # with room the item changes hands, and in the same step goes on from agent 1 to agent 0 again
    prev = _world(C4, pos, tops=('heal', None))
    new = _world(C4, pos, tops=(None, 'heal'))
    L, c, _ = _play(C4, prev, new, [GIVE, NOOP, NOOP, NOOP], [[HEAL], []])
    assert L.stack[0][1] == [HEAL] and c['give_taken'] == 1 and c.get('top_wrong', 0) == 0
    L, c, _ = _play(C4, prev, prev, [GIVE, GIVE, NOOP, NOOP], [[HEAL], []])
    assert L.stack[0][0] == [HEAL] and L.stack[0][1] == [] and c['give_two_hands'] == 1 and c.get('top_wrong', 0) == 0
    # a heal on the ground is nearer than the agent: nothing moves
    prev = _world(C4, pos, tops=('heal', None), heals=[(0.0, 0.9)])
    L, c, _ = _play(C4, prev, prev, [GIVE, NOOP, NOOP, NOOP], [[HEAL], []])
    assert L.stack[0][0] == [HEAL] and c['give_to_heal'] == 1 and c.get('top_wrong', 0) == 0


def test_ledger_places_the_box_ahead_of_the_agent():
    """Agent 0 at (1, 2) facing +y uses a slat: the box stands at (1, 2.75),
    angle 0, with the item's vertices; the heal below it is the new top."""
    item = [SLAT[1], SLAT[2], SLAT[3], SLAT[0]]
    pos = [(1.0, 2.0), FAR[1], FAR[2], FAR[3]]
    ang = [math.pi / 2, 0, 0, 0]
    stack = [[HEAL, (rr.BITEM, _f32bits(item), None)]]
    prev = _world(C4, pos, angle=ang, tops=(item,))
    new = _world(C4, pos, angle=ang, tops=('heal',), boxes=[(item, (1.0, 2.75), 0.0)])
    L, c, st = _play(C4, prev, new, [USE, NOOP, NOOP, NOOP], stack)
    assert c['placements'] == 1 and c['place_q1'] == 1 and c.get('place_wrong', 0) == 0 and st.worst['place_pos'] <= 1.0
    assert L.stack[0][0] == [HEAL] and c.get('top_wrong', 0) == 0 and c.get('conserve_wrong', 0) == 0
    # sin and cos exchanged: the box is a metre off, millions of ulps
    new = _world(C4, pos, angle=ang, tops=('heal',), boxes=[(item, (1.75, 2.0), 0.0)])
    assert _play(C4, prev, new, [USE, NOOP, NOOP, NOOP], stack)[2].worst['place_pos'] > 1e6 > il.TOL['place_pos']
    # the vertices in another order, the box turned: each is no such box
    for box in ((SLAT, (1.0, 2.75), 0.0), (item, (1.0, 2.75), 0.1)):
        new = _world(C4, pos, angle=ang, tops=('heal',), boxes=[box])
        assert _play(C4, prev, new, [USE, NOOP, NOOP, NOOP], stack)[1]['place_wrong'] == 1


def test_ledger_refuses_what_the_rows_have_no_slot_for():
    """Four boxes are all the config has slots for: a fifth is not placed, and
    the item is gone.  Likewise a dropped heal when four lie on the ground."""
    item = [SQUARE[1], SQUARE[2], SQUARE[3], SQUARE[0]]
    boxes = [(SQUARE, (-5.0 + 2 * k, 5.0), 0.0) for k in range(4)]
    pos = [(1.0, 2.0), FAR[1], FAR[2], FAR[3]]
    stack = [[(rr.BITEM, _f32bits(item), None)]]
    prev = _world(C4, pos, tops=(item,), boxes=boxes)
    new = _world(C4, pos, boxes=boxes)
    L, c, _ = _play(C4, prev, new, [USE, NOOP, NOOP, NOOP], stack)
    assert c['spawn_refused'] == 1 and c.get('placements', 0) == 0 and L.stack[0][0] == [] and L.refused_envs == {0}
    assert c.get('place_wrong', 0) == 0 and c.get('conserve_wrong', 0) == 0 and c.get('top_wrong', 0) == 0 and c['conserve_steps'] == 1
    # an engine that keeps the item, or places a fifth box over the fourth's slot
    assert _play(C4, prev, _world(C4, pos, tops=(item,), boxes=boxes), [USE, NOOP, NOOP, NOOP], stack)[1]['top_wrong'] == 1
    moved = boxes[:3] + [(item, (1.75, 2.0), 0.0)]
    assert _play(C4, prev, _world(C4, pos, boxes=moved), [USE, NOOP, NOOP, NOOP], stack)[1]['conserve_wrong'] == 1
    # with three boxes the fourth is placed
    new = _world(C4, pos, boxes=boxes[:3] + [(item, (1.75, 2.0), 0.0)])
    L, c, _ = _play(C4, _world(C4, pos, tops=(item,), boxes=boxes[:3]), new, [USE, NOOP, NOOP, NOOP], stack)
    assert c['placements'] == 1 and c.get('spawn_refused', 0) == 0 and c.get('conserve_wrong', 0) == 0
    # agent 0 dies holding a heal with four heals on the ground: it is not dropped
    heals = [(-5.0 + 2 * k, -5.0) for k in range(4)]
    prev = _world(C4, pos, tops=('heal',), heals=heals, health=[0, 100, 100, 100])
    new = _world(C4, pos, heals=heals, removed=[0])
    L, c, _ = _play(C4, prev, new, [NOOP] * 4, [[HEAL]])
    assert c['spawn_refused'] == 1 and c['deaths_depth1'] == 1 and c.get('conserve_wrong', 0) == 0 and c['conserve_steps'] == 1


def test_ledger_drops_the_stack_at_the_radius():
    """Agent 0, at rest and far from everything, is removed holding a heal
    under a slat: both lie 0.5 m from where it stood, (0.3, 0.4) and (0, -0.5)."""
    item = [SLAT[1], SLAT[2], SLAT[3], SLAT[0]]
    pos = [(2.0, 2.0), FAR[1], FAR[2], FAR[3]]
    stack = [[HEAL, (rr.BITEM, _f32bits(item), None)]]
    prev = _world(C4, pos, tops=(item,), health=[0, 100, 100, 100])
    new = _world(C4, pos, removed=[0], heals=[(2.3, 2.4)], items=[(2.0, 1.5)], item_shapes=[item])
    L, c, st = _play(C4, prev, new, [NOOP] * 4, stack)
    assert c['deaths_depth2'] == 1 and c['drops_free'] == 2 and c['drop_box_items'] == 1 and st.worst['drop_radius'] <= 1.0
    assert c.get('conserve_wrong', 0) == 0 and c.get('drop_wrong', 0) == 0 and L.stack[0][0] == []
    # the heal at the body's own place (radius 0): half a metre off, millions of ulps
    new = _world(C4, pos, removed=[0], heals=[(2.0, 2.0)], items=[(2.0, 1.5)], item_shapes=[item])
    assert _play(C4, prev, new, [NOOP] * 4, stack)[2].worst['drop_radius'] > 1e5 > il.TOL['drop_radius']
    # only the top dropped: the heal is nowhere
    new = _world(C4, pos, removed=[0], items=[(2.0, 1.5)], item_shapes=[item])
    assert _play(C4, prev, new, [NOOP] * 4, stack)[1]['conserve_wrong'] == 1


OWNED = {'agents': {'n_agents': 4, 'agent_size': 1}, 'melee': MELEE,
         'boxes': {'reset_spawns': {'n_boxes': 4, 'box_size': 1}, 'ownership': True, 'item': {'item_size': 0.5, 'offset': 0.75},
                   'health': 20}}


def test_ledger_lets_only_the_owner_break_a_box():
    """Agents 0 and 1 face a box from two sides, 1.4 and 1.6 m away, and swing."""
    C = ir.constants(OWNED)
    item = [SQUARE[1], SQUARE[2], SQUARE[3], SQUARE[0]]
    shape = _f32bits(item)
    pos = [(0.0, 0.0), (3.0, 0.0), FAR[2], FAR[3]]
    ang = [0.0, math.pi, 0.0, 0.0]
    there = _world(C, pos, angle=ang, boxes=[(item, (1.4, 0.0), 0.0)])
    gone = _world(C, pos, angle=ang)
    HIT = (1, 1, 1, 1, 0, 0)
    # a stranger's swing leaves it; the law fails an engine in which it breaks
    L, c, _ = _play(C, there, there, [HIT, NOOP, NOOP, NOOP], [], owners={shape: 1})
    assert c['stranger_swings'] == 1 and c.get('owner_wrong', 0) == 0
    assert _play(C, there, gone, [HIT, NOOP, NOOP, NOOP], [], owners={shape: 1})[1]['owner_wrong'] == 1
    # the owner's swing breaks it, and so does anybody's while it has no owner, which makes that agent the owner
    L, c, _ = _play(C, there, gone, [NOOP, HIT, NOOP, NOOP], [], owners={shape: 1})
    assert c['owner_breaks'] == 1 and c.get('owner_wrong', 0) == 0 and L.owner[0][shape] == 1 and L.due[0][0][1] == shape
    assert _play(C, there, there, [NOOP, HIT, NOOP, NOOP], [], owners={shape: 1})[1]['owner_wrong'] == 1
    L, c, _ = _play(C, there, gone, [HIT, NOOP, NOOP, NOOP], [])
    assert c['free_breaks'] == 1 and L.owner[0][shape] == 0
    # two hitters of different identity in one step: the owner is in doubt
    L, c, _ = _play(C, there, gone, [HIT, HIT, NOOP, NOOP], [])
    assert c['free_breaks'] == 1 and L.owner[0][shape] == il.DOUBT
    # a box nobody swung at does not go
    assert _play(C, there, gone, [NOOP] * 4, [])[1]['box_vanished'] == 1


def test_reset_law_reads_every_property():
    C = C4
    cells = ir.spawn_cells(C)
    boxes = [(SQUARE, tuple(cells[8 + k]), 0.0) for k in range(4)]
    good = dict(heals=[tuple(c) for c in cells[4:8]], boxes=boxes)
    every = np.ones(1, dtype=bool)

    def wrong(**kw):
        st = Stats()
        il.law_reset(C, _world(C, cells[:4], **dict(good, **kw)), every, st)
        return st.count['reset_wrong']

    assert wrong() == 0
    assert wrong(heals=[tuple(cells[0])] + good['heals'][1:]) > 0                           # two bodies on one cell
    assert wrong(heals=[(0.0, 0.0)] + good['heals'][1:]) > 0                                # off the grid
    assert wrong(boxes=[(SQUARE, tuple(cells[8]), 0.5)] + boxes[1:]) > 0                    # a turned box
    assert wrong(boxes=[(np.array(SQUARE)[[1, 2, 3, 0]], tuple(cells[8]), 0.0)] + boxes[1:]) > 0
    assert wrong(boxes=[(SLAT, tuple(cells[8]), 0.0)] + boxes[1:]) > 0                      # not box_size
    assert wrong(health=[100, 100, 99, 100]) > 0 and wrong(tops=('heal',)) > 0 and wrong(boxes=boxes[:3]) > 0


# ---------------------------------------------------------------------------
# the laws on the oracle
# ---------------------------------------------------------------------------
CPU_SEEDS, CPU_STEPS = 8, 300


def oracle_envs(cfg, seeds):
    """(reset, step) of items_laws.run over a list of oracle envs."""
    envs = [oracle.OracleEnv(ResolvedConfig(cfg).to_struct(), pcg64_state(s)) for s in seeds]

    def reset():
        return np.stack([e.reset() for e in envs])

    def step(a):
        out = [e.step(a[k]) for k, e in enumerate(envs)]
        obs = [e.reset() if dn else o for e, (o, _, dn) in zip(envs, out)]
        return np.stack(obs), np.stack([r for _, r, _ in out]), np.array([dn for _, _, dn in out])

    return reset, step


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    sc = il.scenario(name)
    reset, step = oracle_envs(sc.cfg, range(CPU_SEEDS))
    return sc, il.run(sc, reset, step, range(CPU_SEEDS), CPU_STEPS)


@pytest.mark.parametrize('name', il.SCENARIOS + ('loot_ffal',))
def test_oracle_obeys_the_laws(name):
    sc, st = oracle_run(name)
    print(name, st.report())
    il.check(sc, st)


def test_scenarios_cover_teams_ownership_and_both_melee_forms():
    cs = [ir.constants(il.scenario(n).cfg) for n in il.SCENARIOS + ('loot_ffal',)]
    assert {c.cooldown for c in cs if c.ownership} == {0, 40} and {c.teams for c in cs if c.ownership} == {False, True}
    assert {c.randomized for c in cs} == {False, True} and {c.slots for c in cs} == {2, 4, 8}
    assert {c.drop_r for c in cs} == {0.5, 1.0}     # the stock drop radius equals the pickup radius; one scenario tells them apart
