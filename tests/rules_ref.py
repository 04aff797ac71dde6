"""TEST INFRASTRUCTURE ONLY: an fp64 reference of the rules' geometry, written
from the geometry (numpy only): who sees whom, whom a swing hits, what lies
within a radius.  Like physics_ref.py, whose decode, ray casts and wall
polygons it reuses, it never imports the oracle and follows no Box2D operation
order; its inputs are decoded observation rows and the resolved config.

  constants     physics_ref.constants plus the rules' numbers
  decode        physics_ref.decode plus team, zone and inventory-slot columns
  masks         the four visibility mask blocks of every agent's row
  cone          per (camera agent, body): signed distance to the camera polygon
  visible       per (camera agent, body): centre in the cone, first hit, graze
  melee_target  per agent: the closest hit of its swing, graze
  in_radius     point within a circle, graze

Bodies are numbered agents, heals, boxes, box items (A + H + B + B columns).
Every present body occludes: agent circles, heal and box-item circles
(sensors count), box polygons and the four walls; a ray that starts inside a
shape does not hit it (physics_ref.ray_circles / ray_polygons)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import physics_ref as pr
from masurvival.layout import split_obs

NONE, AGENT, HEAL, BOX, BITEM, WALL = -1, 0, 1, 2, 3, 4
STRETCH = 1.0 + 1e-6     # the line-of-sight segment ends this far past the target's centre
MASK_KEYS = ('others_mask', 'heals_mask', 'boxes_mask', 'box_items_mask')


def constants(cfg):
    C = pr.constants(cfg)
    c = C.rc.config
    C.H, C.B, C.teams = C.rc.n_heals, C.rc.n_boxes, C.rc.has_teams
    C.fov, C.depth = float(c['cameras']['fov']), float(c['cameras']['depth'])
    C.melee_range, C.damage = float(c['melee']['range']), int(c['melee']['damage'])
    C.cooldown = 0 if C.rc.continuous_melee else int(c['melee']['cooldown'])
    C.healing, C.slots = int(c['heals']['heal']['healing']), int(c['inventory']['slots'])
    s = c['auto_pickup']['shape']
    C.pickup_r = float(getattr(s, 'radius', s))
    C.zone_damage, C.box_health = int(c['safe_zone']['damage']), int(c['boxes']['health'])
    C.M = C.A + C.H + 2 * C.B
    # body column -> kind, index within the kind
    C.kind = np.concatenate([np.full(C.A, AGENT), np.full(C.H, HEAL), np.full(C.B, BOX), np.full(C.B, BITEM)])
    C.index = np.concatenate([np.arange(C.A), np.arange(C.H), np.arange(C.B), np.arange(C.B)])
    return C


def decode(obs, C):
    """physics_ref.decode of omniscient rows, plus team [N, A], zone [N, 6]
    (centre, radius, next centre, next radius) and each agent's slot blocks:
    heal_slot / box_slot [N, A] True where the top of its inventory is a heal /
    a box item."""
    R = pr.decode(obs, C)
    d = split_obs(np.asarray(obs), C.layout)
    N = R.N
    R.team = d['agent'][..., 1].astype(np.int64) if C.teams else np.broadcast_to(np.arange(C.A), (N, C.A))
    R.zone = d['zone'][:, 0].astype(np.float64)
    R.heal_slot = d['heal_slot_mask'][..., 0] == 0 if 'heal_slot_mask' in d else np.zeros((N, C.A), dtype=bool)
    R.box_slot = d['box_slot_mask'][..., 0] == 0 if 'box_slot_mask' in d else np.zeros((N, C.A), dtype=bool)
    return R


def masks(obs, C):
    """[N, A, M] bool, True where the row's mask says "seen" (0.0), in body
    order; the agent's own column is False.  Also returns the raw blocks."""
    d = split_obs(np.asarray(obs), C.layout)
    N = obs.shape[0]
    seen = np.zeros((N, C.A, C.M), dtype=bool)
    o = d['others_mask'] == 0
    for i in range(C.A):
        seen[:, i, [j for j in range(C.A) if j != i]] = o[:, i]
    k = C.A
    if C.H:
        seen[:, :, k:k + C.H] = d['heals_mask'] == 0
    k += C.H
    if C.B:
        seen[:, :, k:k + C.B] = d['boxes_mask'] == 0
        seen[:, :, k + C.B:k + 2 * C.B] = d['box_items_mask'] == 0
    return seen, {key: d[key] for key in MASK_KEYS if key in d}


def mask_columns(C):
    """bool [D]: the columns of the four mask blocks."""
    m = np.zeros(C.dim, dtype=bool)
    for key in MASK_KEYS:
        if key in C.layout:
            off, shp = C.layout[key]
            m[off:off + int(np.prod(shp))] = True
    return m


def cone_polygon(C):
    """The camera's polygon in the agent's frame, counter-clockwise: the apex,
    depth (cos -fov/2, sin -fov/2), (depth, 0), depth (cos fov/2, sin fov/2)."""
    h = C.fov / 2.0
    return C.depth * np.array([(0.0, 0.0), (np.cos(h), -np.sin(h)), (1.0, 0.0), (np.cos(h), np.sin(h))])


def in_radius(points, centres, radius, graze_eps=1e-4):
    """(inside, graze): |point - centre| <= radius, and |distance - radius| < graze_eps."""
    d = np.asarray(points, dtype=np.float64) - np.asarray(centres, dtype=np.float64)
    dist = np.sqrt((d * d).sum(-1))
    return dist <= radius, np.abs(dist - radius) < graze_eps


def bodies(rows, C):
    """Targets in body order: centres [N, M, 2], there [N, M]."""
    cen = np.concatenate([rows.pos, rows.heals, rows.box_pos, rows.bitems], axis=1)
    on = np.concatenate([rows.present, rows.heals_on, rows.box_on, rows.bitems_on], axis=1)
    return cen, on


def _cast(rows, C, env, p1, d, graze_eps):
    """Rays p1 + t d [K, 2] of envs env [K] against every body of their env.
    Returns (fraction [K, M + 4], graze [K, M + 4]) in body order, then the
    four walls; inf where not hit."""
    N = rows.N
    cen = np.concatenate([rows.pos, rows.heals, rows.bitems], axis=1)
    rad = np.concatenate([np.full(C.A, C.r), np.full(C.H, C.heal_r), np.full(C.B, C.bitem_r)])
    con = np.concatenate([rows.present, rows.heals_on, rows.bitems_on], axis=1)
    poly = np.concatenate([rows.box_world, np.broadcast_to(pr.wall_polygons(C), (N, 4, 4, 2))], axis=1)
    pon = np.concatenate([rows.box_on, np.ones((N, 4), dtype=bool)], axis=1)
    fc, gc = pr.ray_circles(p1, d, cen[env], rad, con[env], graze_eps)
    # only the polygons whose bounding box the ray's own (widened by the band) overlaps can be hit or grazed
    lo, hi = np.minimum(p1, p1 + d) - graze_eps, np.maximum(p1, p1 + d) + graze_eps
    near = pon[env] & (lo[:, None, :] <= poly.max(axis=-2)[env]).all(-1) & (hi[:, None, :] >= poly.min(axis=-2)[env]).all(-1)
    k, m = np.nonzero(near)
    fp, gp = np.full(near.shape, np.inf), np.zeros(near.shape, dtype=bool)
    if len(k):
        f1, g1 = pr.ray_polygons(p1[k], d[k], poly[env[k], m][:, None], np.ones((len(k), 1), dtype=bool), graze_eps)
        fp[k, m], gp[k, m] = f1[:, 0], g1[:, 0]
    a = C.A + C.H
    f = np.concatenate([fc[:, :a], fp[:, :C.B], fc[:, a:], fp[:, C.B:]], axis=1)
    g = np.concatenate([gc[:, :a], gp[:, :C.B], gc[:, a:], gp[:, C.B:]], axis=1)
    return f, g


def _closest(f, length, graze_eps):
    """Column of the least fraction (-1: none) and whether the runner-up lies
    within graze_eps metres of it along the ray."""
    k = f.argmin(axis=1)
    best = np.take_along_axis(f, k[:, None], 1)[:, 0]
    rest = f.copy()
    np.put_along_axis(rest, k[:, None], np.inf, 1)
    with np.errstate(invalid='ignore'):
        tie = np.isfinite(best) & ((rest.min(axis=1) - best) * length < graze_eps)
    return np.where(np.isfinite(best), k, -1), best, tie


def cone(rows, C):
    """The first half of `visible`, no rays cast: (pair, rel, cd) [N, A, M]:
    camera and body both there and distinct, the body's offset from the
    camera, and the signed distance of its centre to the camera polygon placed
    at the agent's pose (negative inside)."""
    cen, on = bodies(rows, C)
    rel = cen[:, None, :, :] - rows.pos[:, :, None, :]
    cd = pr.point_polygon_distance(pr._rot(-rows.angle[:, :, None], rel), cone_polygon(C))
    pair = rows.present[:, :, None] & on[:, None, :]
    pair[:, np.arange(C.A), np.arange(C.A)] = False
    return pair, rel, cd


def visible(rows, C, graze_eps=1e-4):
    """Per camera agent i and body m (arrays [N, A, M]):

      in_cone   the body's centre lies in the camera polygon placed at i's pose
      first     the closest hit of the segment from i's centre to STRETCH times
                the offset of the body's centre is that body
      seen      in_cone & first, for a present camera and a present other body
      graze     the centre is within graze_eps of a cone edge, an occluder is
                within graze_eps of touching or missing the segment, or another
                hit lies within graze_eps of the body's own along the ray
      occluder  kind of the closest hit where it is another body (NONE else)
      pair      camera and body both there and distinct"""
    N, A, M = rows.N, C.A, C.M
    pair, rel, cd = cone(rows, C)
    in_cone = pair & (cd <= 0)
    graze = pair & (np.abs(cd) < graze_eps)
    first = np.zeros((N, A, M), dtype=bool)
    occluder = np.full((N, A, M), NONE)
    n, i, m = np.nonzero(in_cone | graze)
    if len(n):
        p1, d = rows.pos[n, i], STRETCH * rel[n, i, m]
        f, g = _cast(rows, C, n, p1, d, graze_eps)
        length = np.sqrt((d * d).sum(-1))
        k, best, tie = _closest(f, length, graze_eps)
        own = f[np.arange(len(n)), m]
        first[n, i, m] = (k == m) & np.isfinite(own)
        # the body's own hit is not first, but within the band of the closest one
        with np.errstate(invalid='ignore'):
            tie |= np.isfinite(own) & (k != m) & ((own - best) * length < graze_eps)
        graze[n, i, m] |= g.any(axis=1) | tie
        kinds = np.concatenate([C.kind, np.full(4, WALL)])
        occluder[n, i, m] = np.where((k >= 0) & (k != m), kinds[np.maximum(k, 0)], NONE)
    return SimpleNamespace(in_cone=in_cone, first=first, seen=in_cone & first, graze=graze, occluder=occluder,
                              pair=pair, cone_dist=cd, dist=np.sqrt((rel * rel).sum(-1)))


def melee_target(rows, C, graze_eps=1e-4):
    """Per agent [N, A]: kind and index of the closest hit of the segment of
    length melee.range along its heading from its centre (NONE: nothing, or no
    body), `graze` where a body is within graze_eps of touching or missing the
    segment or two hits lie within graze_eps of each other, and reach
    [N, A, A]: the agents whose circle comes within graze_eps of the segment,
    those a grazing swing could hit."""
    N, A = rows.N, C.A
    n, i = np.nonzero(rows.present)
    kind, idx = np.full((N, A), NONE), np.full((N, A), -1)
    graze, reach = np.zeros((N, A), dtype=bool), np.zeros((N, A, A), dtype=bool)
    if len(n):
        ang = rows.angle[n, i]
        p1, d = rows.pos[n, i], C.melee_range * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
        f, g = _cast(rows, C, n, p1, d, graze_eps)
        k, _, tie = _closest(f, C.melee_range, graze_eps)
        kinds = np.concatenate([C.kind, np.full(4, WALL)])
        index = np.concatenate([C.index, np.arange(4)])
        kind[n, i] = np.where(k >= 0, kinds[np.maximum(k, 0)], NONE)
        idx[n, i] = np.where(k >= 0, index[np.maximum(k, 0)], -1)
        graze[n, i] = g.any(axis=1) | tie
        near = pr._seg_point_dist(p1[:, None, :], d[:, None, :], rows.pos[n]) < C.r + graze_eps
        near &= rows.present[n]
        near[np.arange(len(n)), i] = False
        reach[n, i] = near
    return SimpleNamespace(kind=kind, idx=idx, graze=graze, reach=reach)
