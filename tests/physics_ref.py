"""TEST INFRASTRUCTURE ONLY: an fp64 reference of the env's rigid-body step,
written from the physics and the geometry (numpy only).

It never imports the oracle and follows no Box2D operation order.  Everything
it needs is in the omniscient observation rows (every agent's pose and
velocities, heal positions, box vertices and poses, box-item positions), the
actions and the resolved config; walls follow from `floor_size`.

  decode            rows [N, A, D] fp32 -> fp64 arrays [N, A, ...]
  free_flight       next velocity, spin, position, angle of a contact-free agent
  momentum_defect   sum m v' - k^2 (sum m v + sum J) per env
  wall_gaps         centre -> inner face of each wall
  box_gaps          centre -> each present box polygon (negative inside)
  pair_dist / pair_normal_speed
  lidar_ref         closest-hit ray cast against circles and convex polygons
  seek / duel       controllers: pure functions of the decoded rows

The closed forms.  One env step is WORLD_STEPS world steps of H seconds.  The
motor impulse J (body axes, rotated by the agent's angle) acts once, before
the first world step.  Each world step damps the velocity by
k = 1 / (1 + H * DAMPING) and then moves the body by H * v, so with no contact

    v' = (v + R(theta) J / m) k^2          x' = x + H (v + R J / m) (k + k^2)
    w' = (w + Jw / I) k^2                  theta' likewise

with m = DENSITY pi r^2 and I = m r^2 / 2 (a disc).  Contacts between agents
exchange equal and opposite impulses, so sum m v' keeps the same form."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from masurvival.config import ResolvedConfig
from masurvival.layout import obs_layout, split_obs

# not part of the env config: the reference's world constants
H = 1.0 / 60.0           # world step, seconds
WORLD_STEPS = 2          # world steps per env step
DAMPING = 0.8            # linear and angular damping of every agent body
DENSITY = 1.0            # agent fixture density
WALL_ASPECT = 100.0      # ThickRoomWalls: wall length / wall thickness
ACTION_MAP = np.array([-1.0, 0.0, 1.0])


def constants(cfg):
    """The numbers the closed forms need, from the resolved config."""
    rc = cfg if isinstance(cfg, ResolvedConfig) else ResolvedConfig(cfg)
    c = rc.config
    r = float(c['agents']['agent_size']) / 2.0
    m = DENSITY * math.pi * r * r
    floor = float(c['spawn_grid']['floor_size'])
    k = SimpleNamespace(
        rc=rc, A=rc.n_agents, r=r, m=m, I=m * r * r / 2.0, k=1.0 / (1.0 + H * DAMPING),
        impulse=tuple(float(x) for x in c['motors']['impulse']), floor=floor,
        wall_inner=floor / 2.0 - floor / WALL_ASPECT / 2.0,
        heal_r=float(c['heals']['reset_spawns']['item_size']) / 2.0,
        bitem_r=float(c['boxes']['item']['item_size']) / 2.0, lidars=rc.lidars)
    k.dim, k.layout = obs_layout(rc.n_agents, rc.n_heals, rc.n_boxes, rc.has_teams,
                                 int(rc.lidars['n_lasers']) if rc.lidars else 0)
    return k


def wall_polygons(C):
    """World vertices [4, 4, 2] (counter-clockwise) of the four room walls:
    boxes of floor / WALL_ASPECT by floor centred on the room's edges."""
    t, l, o = C.floor / WALL_ASPECT / 2.0, C.floor / 2.0, C.floor / 2.0
    out = []
    for cx, cy, hx, hy in ((-o, 0.0, t, l), (0.0, o, l, t), (o, 0.0, t, l), (0.0, -o, l, t)):
        out.append([(cx - hx, cy - hy), (cx + hx, cy - hy), (cx + hx, cy + hy), (cx - hx, cy + hy)])
    return np.array(out, dtype=np.float64)


def _rot(theta, v):
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c * v[..., 0] - s * v[..., 1], s * v[..., 0] + c * v[..., 1]], axis=-1)


def decode(obs, C):
    """obs fp32 [N, A, D] -> fp64 state arrays.  The omniscient blocks are the
    same in every agent's row; they are read from agent 0's."""
    obs = np.asarray(obs)
    assert obs.ndim == 3 and obs.shape[1:] == (C.A, C.dim), obs.shape
    d = split_obs(obs, C.layout)
    N = obs.shape[0]
    o = 1 + int(C.rc.has_teams)
    ag = d['agent'].astype(np.float64)
    R = SimpleNamespace(N=N, health=ag[..., o], pos=ag[..., o + 1:o + 3], angle=ag[..., o + 3],
                        vel=ag[..., o + 4:o + 6], omega=ag[..., o + 6])
    R.alive = R.health > 0
    # an agent whose health ran out keeps its body for the step in which it is removed: its row still holds
    # a pose then (a removed agent's row is all zero), and it still collides, pushes and stops rays
    R.present = R.alive | (ag[..., o + 1:o + 7] != 0).any(-1)
    if 'heals' in d:
        R.heals = d['heals'][:, 0].astype(np.float64)
        R.heals_on = d['heals_mask'][:, 0] == 0
    else:
        R.heals, R.heals_on = np.zeros((N, 0, 2)), np.zeros((N, 0), dtype=bool)
    if 'boxes' in d:
        b = d['boxes'][:, 0].astype(np.float64)
        R.box_local = b[..., :8].reshape(N, -1, 4, 2)
        R.box_pos, R.box_angle = b[..., 8:10], b[..., 10]
        R.box_on = d['boxes_mask'][:, 0] == 0
        R.box_raw = np.concatenate([d['boxes'][:, 0].reshape(N, -1), d['boxes_mask'][:, 0]], axis=1).view(np.uint32)
        R.bitems = d['box_items'][:, 0, :, 8:10].astype(np.float64)
        R.bitems_on = d['box_items_mask'][:, 0] == 0
    else:
        R.box_local, R.box_pos, R.box_angle = np.zeros((N, 0, 4, 2)), np.zeros((N, 0, 2)), np.zeros((N, 0))
        R.box_on, R.box_raw = np.zeros((N, 0), dtype=bool), np.zeros((N, 0), dtype=np.uint32)
        R.bitems, R.bitems_on = np.zeros((N, 0, 2)), np.zeros((N, 0), dtype=bool)
    R.box_world = _ccw(R.box_pos[:, :, None, :] + _rot(R.box_angle[:, :, None], R.box_local))
    R.lidars = d['lidars'].astype(np.float64) if 'lidars' in d else None
    return R


def _ccw(poly):
    """Vertex loops [..., V, 2] turned counter-clockwise."""
    x, y = poly[..., 0], poly[..., 1]
    area2 = (x * np.roll(y, -1, axis=-1) - np.roll(x, -1, axis=-1) * y).sum(axis=-1)
    return np.where((area2 < 0)[..., None, None], poly[..., ::-1, :], poly)


# ---------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------
def motor_impulse(prev, actions, C):
    """World-frame linear impulse [N, A, 2] and angular impulse [N, A]."""
    a = ACTION_MAP[np.asarray(actions)[..., :3].astype(np.int64)]
    body = np.stack([a[..., 0] * C.impulse[0], a[..., 1] * C.impulse[1]], axis=-1)
    return _rot(prev.angle, body), a[..., 2] * C.impulse[2]


def free_flight(prev, actions, C):
    """(vel, omega, pos, angle) of every agent after one env step without contact."""
    J, Jw = motor_impulse(prev, actions, C)
    v = prev.vel + J / C.m
    w = prev.omega + Jw / C.I
    pos, ang = prev.pos.copy(), prev.angle.copy()
    for _ in range(WORLD_STEPS):
        v = v * C.k
        w = w * C.k
        pos = pos + H * v
        ang = ang + H * w
    return v, w, pos, ang


def momentum_defect(prev, actions, new, C, mask=None):
    """sum m v' - k^2 (sum m v + sum J) per env [N, 2], over the agents of
    `mask` [N, A] (default: alive in both rows)."""
    if mask is None:
        mask = prev.alive & new.alive
    J, _ = motor_impulse(prev, actions, C)
    w = mask[..., None].astype(np.float64)
    before = (w * (C.m * prev.vel + J)).sum(axis=1)
    after = (w * C.m * new.vel).sum(axis=1)
    return after - C.k ** WORLD_STEPS * before


def wall_gaps(rows, C):
    """[N, A, 4]: distance of each alive agent's centre to the inner face of
    the left, top, right and bottom wall (inf for a dead agent)."""
    x, y, e = rows.pos[..., 0], rows.pos[..., 1], C.wall_inner
    g = np.stack([x + e, e - y, e - x, y + e], axis=-1)
    return np.where(rows.alive[..., None], g, np.inf)


def point_polygon_distance(p, poly):
    """Signed distance of points p [..., 2] to convex counter-clockwise
    polygons poly [..., V, 2]: to the nearest boundary point, negative inside."""
    a = poly
    b = np.roll(poly, -1, axis=-2)
    e = b - a
    q = p[..., None, :] - a
    t = np.clip((q * e).sum(-1) / np.maximum((e * e).sum(-1), 1e-300), 0.0, 1.0)
    near = a + t[..., None] * e
    dist = np.sqrt(((p[..., None, :] - near) ** 2).sum(-1)).min(axis=-1)
    side = e[..., 0] * q[..., 1] - e[..., 1] * q[..., 0]  # > 0: left of the edge, the inner side
    inside = (side >= 0).all(axis=-1)
    return np.where(inside, -dist, dist)


def box_gaps(rows, boxes_of=None):
    """[N, A, B]: fp64 distance of each alive agent's centre to each present
    box polygon, negative inside (inf for a dead agent or an empty slot).
    boxes_of: take the boxes from these rows instead (the agents of one row
    against the boxes of the other)."""
    bx = rows if boxes_of is None else boxes_of
    N, A = rows.pos.shape[:2]
    B = bx.box_pos.shape[1]
    if B == 0:
        return np.full((N, A, 0), np.inf)
    d = point_polygon_distance(rows.pos[:, :, None, :], bx.box_world[:, None])
    return np.where(rows.alive[:, :, None] & bx.box_on[:, None, :], d, np.inf)


def pair_dist(rows):
    """[N, A, A] centre distance of the pairs of agent bodies (inf on the
    diagonal and where a body is gone)."""
    d = rows.pos[:, :, None, :] - rows.pos[:, None, :, :]
    dist = np.sqrt((d * d).sum(-1))
    ok = rows.present[:, :, None] & rows.present[:, None, :] & ~np.eye(rows.pos.shape[1], dtype=bool)
    return np.where(ok, dist, np.inf)


def pair_normal_speed(rows):
    """[N, A, A]: (v_j - v_i) . (x_j - x_i) / |x_j - x_i|, positive when the
    pair separates (0 where pair_dist is inf)."""
    d = rows.pos[:, None, :, :] - rows.pos[:, :, None, :]
    dv = rows.vel[:, None, :, :] - rows.vel[:, :, None, :]
    dist = pair_dist(rows)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = (d * dv).sum(-1) / dist
    return np.where(np.isfinite(dist) & (dist > 0), s, 0.0)


# ---------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------
def _seg_point_dist(p1, d, c):
    """distance of points c to the segments p1 + t d, t in [0, 1]"""
    s = c - p1
    t = np.clip((s * d).sum(-1) / np.maximum((d * d).sum(-1), 1e-300), 0.0, 1.0)
    q = s - t[..., None] * d
    return np.sqrt((q * q).sum(-1))


def ray_circles(p1, d, centre, radius, on, graze_eps=1e-4):
    """Rays p1 + t d [..., 2] against circles centre [..., M, 2] (on [..., M]).
    Returns (fraction [..., M], inf where no hit; grazing [..., M]).  The hit
    is the near root of |p1 + t d - c| = r in [0, 1]; a ray that starts inside
    the circle has its near root behind it and hits nothing."""
    p1, d = p1[..., None, :], d[..., None, :]
    s = p1 - centre
    dd = (d * d).sum(-1)
    sd = (s * d).sum(-1)
    disc = sd * sd - dd * ((s * s).sum(-1) - radius * radius)
    with np.errstate(invalid='ignore'):
        t = (-sd - np.sqrt(disc)) / dd
    hit = on & (disc >= 0) & (t >= 0) & (t <= 1)
    near = np.abs(_seg_point_dist(p1, d, centre) - radius) < graze_eps
    near |= np.abs(np.sqrt((s * s).sum(-1)) - radius) < graze_eps
    return np.where(hit, t, np.inf), on & near


def ray_polygons(p1, d, poly, on, graze_eps=1e-4):
    """Rays p1 + t d [..., 2] against convex counter-clockwise polygons
    poly [..., M, V, 2] (on [..., M]).  Returns (fraction [..., M], inf where
    no hit; grazing [..., M]).  The ray is clipped against every face's half
    plane; it hits where it enters the last one, provided that lies in [0, 1]
    and before the first exit.  A ray that starts inside enters no face and
    hits nothing; a ray parallel to a face and outside it misses.  No skin."""
    a = poly
    e = np.roll(poly, -1, axis=-2) - a
    n = np.stack([e[..., 1], -e[..., 0]], axis=-1)  # outward
    n = n / np.maximum(np.sqrt((n * n).sum(-1)), 1e-300)[..., None]  # an empty slot has no edges
    P1, D = p1[..., None, None, :], d[..., None, None, :]
    num = (n * (a - P1)).sum(-1)   # signed distance of the face from the start, < 0: start outside
    den = (n * D).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = num / den
    enter, leave = den < 0, den > 0
    lower = np.where(enter, t, -np.inf).max(axis=-1)
    upper = np.minimum(np.where(leave, t, np.inf).min(axis=-1), 1.0)
    outside_parallel = ((den == 0) & (num < 0)).any(axis=-1)
    hit = on & ~outside_parallel & (lower > 0) & (lower <= upper)
    # grazing: a vertex close to the segment, or an end of the segment close to the boundary
    v_near = (_seg_point_dist(P1, D, a) < graze_eps).any(axis=-1)
    p2 = p1 + d
    ends = (np.abs(point_polygon_distance(p1[..., None, :], poly)) < graze_eps) | \
           (np.abs(point_polygon_distance(p2[..., None, :], poly)) < graze_eps)
    return np.where(hit, lower, np.inf), on & (v_near | ends)


def lidar_endpoints(rows, C):
    """Ray starts [N, A, 2] and ray vectors [N, A, L, 2]."""
    n, fov, depth = int(C.lidars['n_lasers']), float(C.lidars['fov']), float(C.lidars['depth'])
    ang = np.arange(n) * (fov / (n - 1)) - fov / 2.0 + rows.angle[..., None]
    return rows.pos, depth * np.stack([np.cos(ang), np.sin(ang)], axis=-1)


def lidar_ref(rows, C, graze_eps=1e-4):
    """(fraction [N, A, L], grazing [N, A, L]): the relative depth of the
    closest hit of every laser of every agent body, 1.0 where nothing is hit
    (0.0 for a removed agent, as the rows have it).  Agents, heals and box items
    are circles (sensors count), boxes and walls convex polygons.  `grazing`
    marks rays that pass within graze_eps of touching or just missing some
    object, where fp32 may decide hit or miss the other way."""
    p1, d = lidar_endpoints(rows, C)
    N, A, L = d.shape[:3]
    P1 = np.broadcast_to(p1[:, :, None, :], d.shape)
    cen = np.concatenate([rows.pos, rows.heals, rows.bitems], axis=1)
    rad = np.concatenate([np.full(rows.pos.shape[1], C.r), np.full(rows.heals.shape[1], C.heal_r),
                          np.full(rows.bitems.shape[1], C.bitem_r)])
    on = np.concatenate([rows.present, rows.heals_on, rows.bitems_on], axis=1)
    fc, gc = ray_circles(P1, d, cen[:, None, None], rad, on[:, None, None], graze_eps)
    walls = np.broadcast_to(wall_polygons(C), (N, 4, 4, 2))
    poly = np.concatenate([rows.box_world, walls], axis=1)
    pon = np.concatenate([rows.box_on, np.ones((N, 4), dtype=bool)], axis=1)
    fp, gp = ray_polygons(P1, d, poly[:, None, None], pon[:, None, None], graze_eps)
    f = np.minimum(np.minimum(fc.min(axis=-1), fp.min(axis=-1)), 1.0)
    g = gc.any(axis=-1) | gp.any(axis=-1)
    there = rows.present[..., None]
    return np.where(there, f, 0.0), g & there


# ---------------------------------------------------------------------------
# controllers
# ---------------------------------------------------------------------------
SEEK_DEADBAND = 0.05


def seek(rows, targets):
    """int8 actions [N, A, 6]: thrust on both body axes toward targets
    [N, A, 2] (a non-finite target: no thrust), turn at a constant rate."""
    N, A = rows.pos.shape[:2]
    t = np.asarray(targets, dtype=np.float64)
    ok = np.isfinite(t).all(axis=-1) & rows.alive
    body = _rot(-rows.angle, np.where(ok[..., None], t - rows.pos, 0.0))
    a = np.zeros((N, A, 6), dtype=np.int8)
    a[..., 0:2] = 1 + np.sign(np.where(np.abs(body) < SEEK_DEADBAND, 0.0, body)).astype(np.int8)
    a[..., 2] = 2
    a[~rows.alive] = (1, 1, 1, 0, 0, 0)
    return a


def nearest(rows, points, on):
    """[N, A, 2]: for each agent the nearest of points [N, M, 2] with on
    [N, M] or [N, A, M]; nan where there is none."""
    N, A = rows.pos.shape[:2]
    if points.shape[1] == 0:
        return np.full((N, A, 2), np.nan)
    d = points[:, None, :, :] - rows.pos[:, :, None, :]
    dist = np.where(on if on.ndim == 3 else on[:, None, :], (d * d).sum(-1), np.inf)
    k = dist.argmin(axis=-1)
    out = np.take_along_axis(np.broadcast_to(points[:, None], (N, A) + points.shape[1:]), k[..., None, None], axis=2)[:, :, 0]
    return np.where(np.isfinite(dist.min(axis=-1))[..., None], out, np.nan)


def duel(rows):
    """Every agent seeks its nearest living other."""
    A = rows.pos.shape[1]
    on = (rows.alive & rows.present)[:, None, :] & ~np.eye(A, dtype=bool)[None]
    return seek(rows, nearest(rows, rows.pos, on))
