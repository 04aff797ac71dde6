"""fp64 numpy restatement of the scripted bots' rule, written from the text of
include/masurvival.h (mas_bot_act), not from the kernel or masurvival.bots.

``bot_ref(kind, rows, cfg)`` takes observation rows [R, >= obs_dim] whose
values are bf16-representable (so exact in fp64) and the env's config struct
(or anything with its fields) and returns (actions int8 [R, 6], near bool [R]).

near: a row on which some geometric comparison ``l > r`` the rule evaluated
had |l - r| <= 1e-4 * max(1, |l|, |r|): the kernel's fp32 arithmetic may
decide it the other way, so such a row is not compared.  Comparisons of
exactly representable quantities (masks, health against its threshold, team
ids) are exact on both sides and never set the flag; so is the tie of two
targets that mirror each other about the agent (see _nearest: agents and heals
spawn on a grid, so such ties open most episodes).  Any other exact tie
(l == r) sets the flag as the definition says.
"""
import numpy as np

from masurvival.layout import obs_layout

IDLE, HUNTER, FORAGER = 0, 1, 2
KINDS = {'idle': IDLE, 'hunter': HUNTER, 'forager': FORAGER}

# the constants of the header's rule text
ZONE_MARGIN = 1.0
TURN_BAND = 0.15
TURN_DAMP = 0.25
MOVE_CONE = 0.8
ATTACK_CONE = 0.9
STANDOFF = 1.25
ARRIVED = 0.25
FORAGER_FIGHT = 4.0
NEAR_BAND = 1e-4


def _near(l, r):
    return np.abs(l - r) <= NEAR_BAND * np.maximum(1.0, np.maximum(np.abs(l), np.abs(r)))


def _nearest(dx, dy, valid):
    """Index of the least dx^2 + dy^2 among valid (lowest index on a tie), whether
    any is valid, whether another valid candidate lies within the band of it,
    and the squared distances.  A candidate that mirrors the best one (the same
    two |dx|, |dy|, in either order) gives the same bits as it in any
    arithmetic: that tie is exact on both sides and sets no flag."""
    d2 = dx * dx + dy * dy
    big = np.where(valid, d2, np.inf)
    k = np.argmin(big, axis=1)  # the first least: the lowest index
    has = valid.any(axis=1)
    best = np.take_along_axis(big, k[:, None], 1)
    best0 = np.where(has[:, None], best, 0.0)
    ax, ay = np.abs(dx), np.abs(dy)
    bx, by = np.take_along_axis(ax, k[:, None], 1), np.take_along_axis(ay, k[:, None], 1)
    mirror = ((ax == bx) & (ay == by)) | ((ax == by) & (ay == bx))
    close = (valid & ~mirror & _near(np.where(valid, d2, 0.0), best0)).any(axis=1)
    return k, has, close & has, d2


def bot_ref(kind, rows, cfg):
    rows = np.asarray(rows, dtype=np.float64)
    R = rows.shape[0]
    A, H, teams = int(cfg.n_agents), int(cfg.n_heals), int(bool(cfg.teams))
    _, lay = obs_layout(A, H, int(cfg.n_boxes), bool(teams), int(getattr(cfg, 'lidar_n_lasers', 0)))
    rec = 8 + teams
    o = 1 + teams  # health's index in an agent record: [id, (team), health, x, y, angle, vx, vy, w]
    ag = rows[:, lay['agent'][0]:lay['agent'][0] + rec]
    hp, px, py, th, w = ag[:, o], ag[:, o + 1], ag[:, o + 2], ag[:, o + 3], ag[:, o + 6]
    zo = lay['zone'][0]
    zx, zy, zr = rows[:, zo], rows[:, zo + 1], rows[:, zo + 2]
    acts = np.zeros((R, 6), dtype=np.int8)
    acts[:, :3] = 1
    near = np.zeros(R, dtype=bool)
    if kind == IDLE:
        return acts, near
    live = hp > 0
    if H > 0:
        hsm = rows[:, lay['heal_slot_mask'][0]]
        acts[:, 4] = live & (hsm == 0) & (hp <= float(int(cfg.agent_health) - int(cfg.healing)))

    # 1. outside the zone
    ex, ey = px - zx, py - zy
    q = ex * ex + ey * ey
    m = np.maximum(zr - ZONE_MARGIN, 0.0)
    outside = q > m * m
    near |= live & _near(q, m * m)
    tk = np.where(outside, 1, 0)  # 0 none, 1 zone, 2 heal, 3 enemy
    tx, ty = np.where(outside, zx, 0.0), np.where(outside, zy, 0.0)

    # 2. FORAGER: the nearest visible heal
    if kind == FORAGER and H > 0:
        hs = rows[:, lay['heals'][0]:lay['heals'][0] + 2 * H].reshape(R, H, 2)
        hv = rows[:, lay['heals_mask'][0]:lay['heals_mask'][0] + H] == 0
        # (only heals inside the zone's margin: not |heal - zone_c|^2 > m^2)
        gx, gy = hs[:, :, 0] - zx[:, None], hs[:, :, 1] - zy[:, None]
        gq, mm = gx * gx + gy * gy, (m * m)[:, None]
        near |= live & (tk == 0) & (hv & _near(gq, mm)).any(axis=1)
        hv &= ~(gq > mm)
        dx, dy = hs[:, :, 0] - px[:, None], hs[:, :, 1] - py[:, None]
        k, has, close, _ = _nearest(dx, dy, hv)
        take = (tk == 0) & has
        near |= live & take & close
        tk = np.where(take, 2, tk)
        tx = np.where(take, hs[np.arange(R), k, 0], tx)
        ty = np.where(take, hs[np.arange(R), k, 1], ty)

    # 3. the nearest visible living enemy
    ot = rows[:, lay['others'][0]:lay['others'][0] + (A - 1) * rec].reshape(R, A - 1, rec)
    ov = (rows[:, lay['others_mask'][0]:lay['others_mask'][0] + A - 1] == 0) & (ot[:, :, o] > 0)
    if teams:
        ov &= ot[:, :, 1] != ag[:, 1][:, None]
    dx, dy = ot[:, :, o + 1] - px[:, None], ot[:, :, o + 2] - py[:, None]
    k, has, close, d2 = _nearest(dx, dy, ov)
    cand = (tk == 0) & has
    near |= live & cand & close
    if kind == FORAGER:
        best = d2[np.arange(R), k]
        lim = FORAGER_FIGHT * FORAGER_FIGHT
        near |= live & cand & _near(best, lim)
        cand &= ~(best > lim)
    tk = np.where(cand, 3, tk)
    tx = np.where(cand, ot[np.arange(R), k, o + 1], tx)
    ty = np.where(cand, ot[np.arange(R), k, o + 2], ty)

    # steering
    dx, dy = tx - px, ty - py
    dist = np.sqrt(dx * dx + dy * dy)
    hx, hy = np.cos(th), np.sin(th)
    c = hx * dx + hy * dy
    s = hx * dy - hy * dx
    u = s - TURN_DAMP * w * dist
    band = TURN_BAND * dist
    has_t = live & (tk != 0)
    enemy = tk == 3
    left = u > band
    right = ~left & (-band > u)
    back = ~left & ~right & (0.0 > c)
    turn = np.where(left | back, 2, np.where(right, 0, 1))
    near |= has_t & _near(u, band)
    near |= has_t & ~left & _near(-band, u)
    near |= has_t & ~left & ~right & _near(0.0, c)
    ahead = c > MOVE_CONE * dist
    near |= has_t & _near(c, MOVE_CONE * dist)
    stop = np.where(enemy, STANDOFF, ARRIVED)
    close_in = ~(dist > stop)
    near |= has_t & ahead & _near(dist, stop)
    reach = float(cfg.melee_range) + float(cfg.agent_size) / 2.0
    in_reach = enemy & ~(dist > reach)
    near |= has_t & enemy & _near(dist, reach)
    hit = in_reach & (c > ATTACK_CONE * dist)
    near |= has_t & in_reach & _near(c, ATTACK_CONE * dist)

    acts[:, 0] = np.where(has_t & ahead & ~close_in, 2, 1)
    acts[:, 2] = np.where(has_t, turn, 2)  # 5. no target: turn counter-clockwise in place
    acts[:, 3] = has_t & hit
    # a dead self: the no-op
    acts[~live] = np.array([1, 1, 1, 0, 0, 0], dtype=np.int8)
    near &= live
    return acts, near
