"""TEST INFRASTRUCTURE ONLY: an fp64 reference of where items go, written from
the reference's text (GiveLast, Inventory, DeathDrop, ObjectItem.use,
OwnedObjectItem, SpawnGrid, RandomizeBoxShapes, shape_query), numpy only.  Like
physics_ref.py and rules_ref.py, whose decode, in_radius and free flight it
reuses, it never imports the oracle; its inputs are decoded observation rows,
the actions and the resolved config.

  constants     rules_ref.constants plus the give, drop, placing and grid numbers
  decode        rules_ref.decode plus the fp32 bits of every shape a row shows
  give_taker    per agent: the nearest body whose centre lies in the give circle
  placement     pos + offset (cos angle, sin angle)
  spawn_cells   the grid_size^2 cell centres of the spawn grid
  rect_dims     width, height and form of a box's four local vertices
  item_shape    the vertex loop of a broken box's item
  corpse        where a dying agent's body is when it is removed
  max_step      the farthest an agent's centre can move in one env step

A query (shape_query) returns the bodies whose centre lies in the circle placed
at the agent's centre, out of every body of the world: agents, heals, boxes,
box items and the four walls, whose centres lie on the room's edges."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import physics_ref as pr
import rules_ref as rr
from masurvival.layout import split_obs
from physics_laws import FAT

NONE, AGENT, HEAL, BOX, BITEM, WALL = rr.NONE, rr.AGENT, rr.HEAL, rr.BOX, rr.BITEM, rr.WALL
PLACED, DUE = 5, 6          # extra bodies: a box placed earlier in this step, a due item just spawned
MAX_LINEAR_CORRECTION = 0.2  # Box2D: the most a position solver moves a body per world step


def constants(cfg):
    C = rr.constants(cfg)
    c = C.rc.config
    s = c['give']['shape']
    C.give_r = float(getattr(s, 'radius', s))
    C.drop_r = float(c['death_drop']['radius'])
    C.offset = float(c['boxes']['item']['offset'])
    C.grid = int(c['spawn_grid']['grid_size'])
    C.box_size = float(c['boxes']['reset_spawns'].get('box_size', 1))
    rs = c['boxes'].get('randomized_shape')
    C.randomized = rs is not None
    C.min_w, C.min_h = (float(rs.get('min_w', 0.1)), float(rs.get('min_h', 0.1))) if rs else (0.1, 0.1)
    C.ownership = bool(c['boxes'].get('ownership', False))
    C.full_health = int(c['health']['health'])
    C.zone_r0 = float(c['safe_zone']['radiuses'][0])
    return C


def decode(obs, C):
    """rules_ref.decode plus, as uint32 bits: box_bits [N, B, 8] and bitem_bits
    [N, B, 8], the local vertices of every box and of every box item on the
    ground, top_bits [N, A, 8], the `box_slot` block, box_item_bits [N, B, 8],
    item_shape of every box; heal_amount [N, A], the `heal_slot` block;
    slot_raw [N, A, 2], the two slot masks as written."""
    R = rr.decode(obs, C)
    obs = np.ascontiguousarray(np.asarray(obs, dtype=np.float32))
    d = split_obs(obs, C.layout)
    N = R.N
    if C.B:
        R.box_bits = np.ascontiguousarray(d['boxes'][:, 0, :, :8]).view(np.uint32)
        R.bitem_bits = np.ascontiguousarray(d['box_items'][:, 0, :, :8]).view(np.uint32)
        R.top_bits = np.ascontiguousarray(d['box_slot'][:, :, 0, :]).view(np.uint32)
        bm = d['box_slot_mask'][..., 0]
    else:
        R.box_bits = R.bitem_bits = np.zeros((N, 0, 8), dtype=np.uint32)
        R.top_bits, bm = np.zeros((N, C.A, 8), dtype=np.uint32), np.ones((N, C.A), dtype=np.float32)
    if C.H:
        R.heal_amount, hm = d['heal_slot'][:, :, 0, 0].astype(np.float64), d['heal_slot_mask'][..., 0]
    else:
        R.heal_amount, hm = np.zeros((N, C.A)), np.ones((N, C.A), dtype=np.float32)
    R.slot_raw = np.stack([hm, bm], axis=-1).astype(np.float64)
    R.box_item_bits = item_shapes(R.box_bits)
    return R


def wall_centres(C):
    """[4, 2]: the centres of the left, top, right and bottom wall."""
    o = C.floor / 2.0
    return np.array([(-o, 0.0), (0.0, o), (o, 0.0), (0.0, -o)])


def no_extra(N):
    return SimpleNamespace(pos=np.zeros((N, 0, 2)), on=np.zeros((N, 0), dtype=bool), kind=np.zeros((N, 0), dtype=np.int64),
                           idx=np.zeros((N, 0), dtype=np.int64))


def give_taker(rows, C, extra_bodies=None, graze_eps=1e-4):
    """Per agent [N, A]: kind and index (within the kind) of the body whose
    centre is nearest to the agent's centre among the bodies, other than the
    agent itself, whose centre lies within the give radius; NONE, -1 where
    there is none or the agent is not there.  The bodies are the present
    agents, heals, boxes, box items, the four walls' centres and extra_bodies
    (pos [N, E, 2], on [N, E], kind [N, E], idx [N, E]): what is in the world
    before GiveLast runs and in no row.  `graze`: a centre within graze_eps of
    the radius, or the two least distances within graze_eps of each other;
    reach [N, A, A]: the agents within the radius + graze_eps, those a grazing
    give could go to."""
    N, A = rows.N, C.A
    X = no_extra(N) if extra_bodies is None else extra_bodies
    cen, on = rr.bodies(rows, C)
    cen = np.concatenate([cen, np.broadcast_to(wall_centres(C), (N, 4, 2)), X.pos], axis=1)
    on = np.concatenate([on, np.ones((N, 4), dtype=bool), X.on], axis=1)
    kinds = np.concatenate([np.broadcast_to(np.concatenate([C.kind, np.full(4, WALL)]), (N, C.M + 4)), X.kind], axis=1)
    index = np.concatenate([np.broadcast_to(np.concatenate([C.index, np.arange(4)]), (N, C.M + 4)), X.idx], axis=1)
    d = cen[:, None, :, :] - rows.pos[:, :, None, :]
    dist = np.sqrt((d * d).sum(-1))                                    # [N, A, M']
    pair = rows.present[:, :, None] & on[:, None, :]
    pair[:, np.arange(A), np.arange(A)] = False
    inside = pair & (dist <= C.give_r)
    rim = pair & (np.abs(dist - C.give_r) < graze_eps)
    cand = np.where(inside, dist, np.inf)
    k = cand.argmin(-1)
    best = np.take_along_axis(cand, k[..., None], -1)[..., 0]
    rest = cand.copy()
    np.put_along_axis(rest, k[..., None], np.inf, -1)
    with np.errstate(invalid='ignore'):
        tie = np.isfinite(best) & (rest.min(-1) - best < graze_eps)
    some = np.isfinite(best)
    kind = np.where(some, np.take_along_axis(kinds[:, None, :].repeat(A, 1), k[..., None], -1)[..., 0], NONE)
    idx = np.where(some, np.take_along_axis(index[:, None, :].repeat(A, 1), k[..., None], -1)[..., 0], -1)
    reach = pair[:, :, :A] & (dist[:, :, :A] < C.give_r + graze_eps)
    return SimpleNamespace(kind=kind, idx=idx, graze=rim.any(-1) | tie, reach=reach, dist=np.where(some, best, np.inf))


def placement(pos, angle, offset):
    """pos + offset (cos angle, sin angle): from_polar is R(angle) (length, 0)."""
    pos, angle = np.asarray(pos, dtype=np.float64), np.asarray(angle, dtype=np.float64)
    return pos + offset * np.stack([np.cos(angle), np.sin(angle)], axis=-1)


def spawn_cells(C):
    """[grid^2, 2]: cell k has its centre at column k % grid, row k // grid of
    a grid of floor / grid squares centred on the room."""
    g, f = C.grid, C.floor
    c = f * ((np.arange(g) + 0.5) / g) - f / 2.0
    k = np.arange(g * g)
    return np.stack([c[k % g], c[k // g]], axis=-1)


def rect_dims(local_vertices):
    """(w, h, ok) of vertex loops [..., 4, 2]: w and h from the first and the
    second edge; ok where the loop is exactly (-w/2, -h/2), (w/2, -h/2),
    (w/2, h/2), (-w/2, h/2): centred, axis-aligned and in SetAsBox order."""
    v = np.asarray(local_vertices, dtype=np.float64)
    w, h = v[..., 1, 0] - v[..., 0, 0], v[..., 2, 1] - v[..., 1, 1]
    want = np.stack([np.stack([-w / 2, -h / 2], -1), np.stack([w / 2, -h / 2], -1),
                     np.stack([w / 2, h / 2], -1), np.stack([-w / 2, h / 2], -1)], axis=-2)
    return w, h, (v == want).all((-1, -2)) & (w > 0) & (h > 0)


def item_shape(bits):
    """The 8 fp32 bit patterns of a broken box's item, given the box's: the
    item keeps a copy of the box's polygon made from its vertex list
    (simulation.prototype -> copy_shape -> b2PolygonShape(vertices=...)), and
    Box2D rebuilds such a polygon as the hull that starts at the rightmost
    vertex, the lower one on a tie, and runs counter-clockwise.  For a loop in
    SetAsBox order that is the same loop started at (w/2, -h/2); a loop already
    in that form is unchanged, so a box placed from an item and broken again
    yields the same 8 floats."""
    return tuple(item_shapes(np.array(bits, dtype=np.uint32)).tolist())


def item_shapes(bits):
    """item_shape of every row of bits [..., 8] (uint32), as an array."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    v = bits.view(np.float32).reshape(bits.shape[:-1] + (4, 2))
    x, y = v[..., 0], v[..., 1]
    k = np.where(x == x.max(-1, keepdims=True), y, np.inf).argmin(-1)
    idx = (k[..., None] + np.arange(4)) % 4
    out = np.take_along_axis(bits.reshape(bits.shape[:-1] + (4, 2)), idx[..., None], axis=-2)
    return out.reshape(bits.shape)


def max_step(prev, C, actions):
    """[N]: no agent's centre moves farther than this in one env step.  Contacts
    between the agents (equal masses) create no kinetic energy, so no speed
    exceeds the sum of the speeds the motors leave; each world step may add one
    position correction."""
    J, _ = pr.motor_impulse(prev, actions, C)
    v = prev.vel + J / C.m
    speed = (np.sqrt((v * v).sum(-1)) * prev.present).sum(-1)
    return pr.WORLD_STEPS * (pr.H * speed + MAX_LINEAR_CORRECTION)


def corpse(prev, C, actions, new=None):
    """(pos [N, A, 2], free [N, A]): where each agent's body is at the end of
    the step by law 1's closed form on the previous row, and whether that
    agent-step is free flight under law 1's margin test: no wall, box or other
    agent body within the broad-phase margin at either end of the step.  The
    others and the boxes are taken from the previous row and, if given, from
    the new one too (a removed agent's own row is zeroed there, which is why
    its last position has to be computed)."""
    _, _, pos, _ = pr.free_flight(prev, actions, C)
    A = C.A
    ends = SimpleNamespace(pos=pos, alive=prev.present, present=prev.present)
    start = SimpleNamespace(pos=prev.pos, alive=prev.present, present=prev.present)
    gaps = [pr.wall_gaps(start, C), pr.wall_gaps(ends, C)]
    worlds = [prev] if new is None else [prev, new]
    for w in worlds:
        gaps += [pr.box_gaps(start, w), pr.box_gaps(ends, w)]
    near = np.concatenate(gaps, -1).min(-1) < C.r + FAT
    others = [(prev.pos, prev.present), (pos, prev.present)] + ([] if new is None else [(new.pos, new.present)])
    for p in (prev.pos, pos):
        for q, on in others:
            d = p[:, :, None, :] - q[:, None, :, :]
            dist = np.where(on[:, None, :] & ~np.eye(A, dtype=bool)[None], np.sqrt((d * d).sum(-1)), np.inf)
            near |= dist.min(-1) < 2 * C.r + FAT
    return pos, prev.present & ~near
