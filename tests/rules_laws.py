"""TEST INFRASTRUCTURE ONLY: the laws the rules' geometry must obey (who sees
whom, whom a swing hits, which item is picked up, who stands outside the zone),
the scenarios that drive envs into those regimes, and the loop that applies
the one to the other.  Shared by tests/test_rules_reference.py (the C oracle,
CPU) and tests/test_gpu_rules_laws.py (the HIP kernels).

Ground truth for hidden state comes from a twin: the same config with
observation.omniscent True and False, the same seeds, the same actions.  The
omniscient twin's rows give every body's pose (rules_ref.decode); the other
twin's masks are what is judged.  Every decision here is exact (a mask, an
integer health, an item there or gone), so there is no tolerance: a case
within LIDAR_GRAZE of the geometric threshold is excused and counted, every
other disagreement is an error.

The engine's own "alive" is `present` in the decoded rows: an agent whose
health ran out after the despawn pass (zone damage) keeps its body, acts, is
hit, picks up and sees for one more step."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import physics_ref as pr
import rules_ref as rr
from masurvival.config import C1_CONFIG, C3_CONFIG, C5_CONFIG
from physics_laws import LIDAR_GRAZE, LIDAR_GRAZE_SHARE, Stats

BAND = LIDAR_GRAZE
VIS_SKIP_SHARE = 0.5      # law B may skip at most this share of env-steps
LEDGER_SKIP_SHARE = 0.05  # law C may exclude at most this share of agent-steps
RIM = 0.2                 # coverage: an agent this close to the zone's rim is at the rim
MASK_BLOCKS = ('others', 'heals', 'boxes', 'box_items')


def _same_items(a_pos, a_on, b_pos, b_on):
    """[N, Ma]: item k of a (there) has an item of b (there) at the same fp32 position."""
    eq = (a_pos[:, :, None, :] == b_pos[:, None, :, :]).all(-1) & b_on[:, None, :]
    return a_on & eq.any(-1)


def _same_boxes(a, b):
    """[N, B]: box k of rows a has a box of rows b with the same vertices and pose."""
    eq = (a.box_pos[:, :, None, :] == b.box_pos[:, None, :, :]).all(-1)
    eq &= a.box_angle[:, :, None] == b.box_angle[:, None, :]
    eq &= (a.box_local[:, :, None] == b.box_local[:, None, :]).all((-1, -2))
    return a.box_on & (eq & b.box_on[:, None, :]).any(-1)


class State:
    """What the laws carry from step to step, per env: each agent's melee
    cooldown as an interval [cd_lo, cd_hi], its inventory depth and whether
    that is known, and the positions of boxes broken in the last step, whose
    items are due at the start of the next."""

    def __init__(self, N, C):
        self.cd_lo = np.zeros((N, C.A), dtype=np.int64)
        self.cd_hi = np.zeros((N, C.A), dtype=np.int64)
        self.depth = np.zeros((N, C.A), dtype=np.int64)
        self.known = np.ones((N, C.A), dtype=bool)
        self.due = [[] for _ in range(N)]

    def reset(self, envs):
        for a in (self.cd_lo, self.cd_hi, self.depth):
            a[envs] = 0
        self.known[envs] = True
        for n in np.nonzero(envs)[0]:
            self.due[n] = []


# ---------------------------------------------------------------------------
# law A
# ---------------------------------------------------------------------------
def law_twins(C, omni, non, st):
    """Law A: outside the four mask blocks the twins agree bit for bit, in
    every row (reset rows included), every reward and every done flag."""
    (oo, ro, do), (on, rn, dn) = omni, non
    keep = ~rr.mask_columns(C)
    bad = (np.asarray(oo)[..., keep].view(np.uint32) != np.asarray(on)[..., keep].view(np.uint32)).sum()
    if ro is not None:
        bad += (np.asarray(ro).view(np.uint32) != np.asarray(rn).view(np.uint32)).sum()
        bad += (np.asarray(do, dtype=bool) != np.asarray(dn, dtype=bool)).sum()
    st.add('twin_diffs', bad)
    st.add('twin_rows', oo.shape[0])


# ---------------------------------------------------------------------------
# law B
# ---------------------------------------------------------------------------
def unchanged(prev, new):
    """[N]: the present agents and the heals, boxes and box_items blocks are
    the same in both rows."""
    same = (prev.present == new.present).all(-1)
    same &= (prev.heals_on == new.heals_on).all(-1) & (np.where(prev.heals_on[..., None], prev.heals, 0) ==
                                                      np.where(new.heals_on[..., None], new.heals, 0)).all((-1, -2))
    same &= (prev.box_raw == new.box_raw).all(-1)
    same &= (prev.bitems_on == new.bitems_on).all(-1) & (np.where(prev.bitems_on[..., None], prev.bitems, 0) ==
                                                        np.where(new.bitems_on[..., None], new.bitems, 0)).all((-1, -2))
    return same


def law_visibility(C, rows, obs_non, judged, st, t):
    """Law B: a mask is 0 exactly when the body's centre lies in the camera's
    cone and the line of sight's first hit is that body.

    The cameras run after the physics and the breaking of boxes, but before
    dead agents are removed, dropped items appear and items are picked up; the
    row is written after all of that, with each camera's list read at the
    agent's index among the survivors.  So the row shows what the cameras saw
    only when nothing came or went in between: a step is judged when the set
    of present agents and the heals, boxes and box_items blocks are the same
    as in the previous row (then the new row's bodies are exactly the
    occluders the cameras had), and every reset row is judged, where the
    cameras run on the world as dealt.  A step at whose start a broken box's
    item was due is not judged either: had the item been picked up in that very
    step, it would have stood in the cameras' way and be in neither row.  The
    rest are counted as vis_skipped.
    A body that is not there, a camera that is not there and the agent itself
    read 1 in every row, judged or not."""
    seen, _ = rr.masks(obs_non, C)
    V = rr.visible(rows, C, BAND)
    st.add('vis_phantom', (seen & ~V.pair).sum())
    J = judged[:, None, None] & V.pair
    wrong = J & (seen != V.seen)
    st.add('vis_pairs', J.sum())
    st.add('vis_graze', (J & V.graze).sum())
    st.add('vis_excused', (wrong & V.graze).sum())
    st.add('vis_wrong', (wrong & ~V.graze).sum())
    if (wrong & ~V.graze).any() and 'vis_wrong' not in st.where:
        st.where['vis_wrong'] = (t,) + tuple(int(x[0]) for x in np.nonzero(wrong & ~V.graze))
    st.add('vis_judged_steps', judged.sum())
    st.add('vis_skipped', (~judged).sum())
    # coverage
    ok = J & ~V.graze
    hidden = ok & V.in_cone & ~V.first
    st.add('vis_seen', (ok & V.seen).sum())
    st.add('occ_box', (hidden & (V.occluder == rr.BOX)).sum())
    st.add('occ_agent', (hidden & (V.occluder == rr.AGENT)).sum())
    st.add('occ_item', (hidden & ((V.occluder == rr.HEAL) | (V.occluder == rr.BITEM))).sum())
    st.add('out_of_cone_near', (ok & ~V.in_cone & (V.dist < C.depth * np.cos(C.fov / 2.0))).sum())
    item = (C.kind == rr.HEAL) | (C.kind == rr.BITEM)
    st.add('cam_inside_item', (hidden & item[None, None, :] & (V.occluder == rr.NONE)).sum())
    st.add('items_seen', (ok & V.seen & item[None, None, :]).sum())
    st.add('items_hidden', (hidden & item[None, None, :]).sum())
    st.worst['max_in_cone'] = max(st.worst.get('max_in_cone', 0), int(V.in_cone.sum(-1).max()) if V.in_cone.size else 0)
    k = 0
    for name, width in zip(MASK_BLOCKS, (C.A, C.H, C.B, C.B)):
        blk, pr_ = seen[:, :, k:k + width], J[:, :, k:k + width]
        st.add(f'mask0_{name}', (pr_ & blk).sum())
        st.add(f'mask1_{name}', (pr_ & ~blk).sum())
        k += width
    return V


# ---------------------------------------------------------------------------
# law C
# ---------------------------------------------------------------------------
def law_ledger(C, prev, new, actions, valid, L, st, t):
    """Law C: for every agent present in both rows, health' - health is
    -damage x (attackers whose swing's closest hit is that agent, who pressed
    attack, are off cooldown and not of its team) + healing (use pressed with a
    heal on top of the inventory) - zone damage (new position outside the
    previous row's zone circle, or the endgame: a zone of radius 0).  A box
    that such a swing hits is gone from the next row, a box no swing can have
    hit is still there, and a broken box's item appears at its position one
    step later.

    The swing is cast in the previous row's world, before the physics.  Two
    things that world holds are in neither row: a box placed by `use` in this
    step (it is placed before the swings, and the new row shows it after the
    physics pushed agents about), and the item of a box broken in the step
    before, which appears at the start of this step.  Env-steps with a placed
    box are excluded whole.  A due item is a circle of the item's radius at
    the broken box's position, which the law remembers, so there only the
    swings that come within BAND of that circle are in doubt.  For a swing in
    doubt, as for one within BAND of touching or missing something, every
    agent it could reach is left unjudged (ledger_excluded) and the swinger's
    cooldown becomes an interval, narrowed again from what is observed (a hit
    that shows, or does not, on an agent or a box nobody else touched)."""
    N, A = prev.N, C.A
    a = np.asarray(actions)
    alive0, alive1 = prev.present, new.present
    T = rr.melee_target(prev, C, BAND)
    placed = (alive0 & (a[..., 4] == 1) & prev.box_slot).any(-1)
    due_pos = L.due
    due = np.array([len(d) > 0 for d in due_pos])
    # a due item is a circle at the broken box's position: only a swing that comes within BAND of it is in doubt
    near_due = np.zeros((N, A), dtype=bool)
    for n in np.nonzero(due)[0]:
        ang = prev.angle[n][:, None]
        d = C.melee_range * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
        gap = pr._seg_point_dist(prev.pos[n][:, None, :], d, np.array(due_pos[n])[None, :, :])
        near_due[n] = (gap < C.bitem_r + BAND).any(-1)
    blind = placed[:, None] | near_due
    graze = T.graze | blind
    reach = np.where(blind[:, :, None], alive0[:, None, :] & ~np.eye(A, dtype=bool)[None], T.reach)
    pressed = alive0 & (a[..., 3] == 1)
    hit_any = T.kind != rr.NONE
    sure = pressed & hit_any & ~graze & (L.cd_hi == 0)
    maybe = pressed & (hit_any | graze) & (L.cd_lo == 0) & ~sure
    swings = SimpleNamespace(T=T, sure=sure, maybe=maybe.copy(), graze=graze, ready=L.cd_hi == 0)   # for items_laws (law K)
    at_agent = (T.kind == rr.AGENT)[:, :, None] & (T.idx[:, :, None] == np.arange(A)[None, None, :])   # [N, i, j]
    foe = prev.team[:, :, None] != prev.team[:, None, :]
    hits = (sure[:, :, None] & at_agent & foe).sum(1)
    touched = (maybe[:, :, None] & np.where(graze[:, :, None], reach, at_agent & foe))            # [N, i, j]
    unsure = touched.any(1)
    used = alive0 & (a[..., 4] == 1) & prev.heal_slot
    endgame = prev.zone[:, 2] == 0
    inside, zg = rr.in_radius(new.pos, prev.zone[:, None, 0:2], prev.zone[:, None, 2], BAND)
    outside = ~inside | endgame[:, None]
    unsure |= zg & ~endgame[:, None]
    both = alive0 & alive1 & valid[:, None]
    expect = -C.damage * hits + C.healing * used - C.zone_damage * outside
    resid = (new.health - prev.health) - expect
    judged = both & ~unsure
    bad = judged & (resid != 0)
    st.add('ledger_steps', both.sum())
    st.add('ledger_excluded', (both & unsure).sum())
    st.add('ledger_wrong', bad.sum())
    if bad.any() and 'ledger_wrong' not in st.where:
        st.where['ledger_wrong'] = (t,) + tuple(int(x[0]) for x in np.nonzero(bad))
    # coverage
    st.add('agent_hits', (hits * judged).sum())
    st.add('team_swings', (sure[:, :, None] & at_agent & ~foe & valid[:, None, None]).sum())
    st.add('heal_uses', (used & judged).sum())
    st.add('zone_out_rim', (judged & outside & ~endgame[:, None] & _near_rim(new, prev)).sum())
    st.add('zone_in_rim', (judged & ~outside & _near_rim(new, prev)).sum())
    st.add('zone_endgame', (judged & endgame[:, None]).sum())
    st.add('deaths', (alive0 & ~alive1 & valid[:, None]).sum())
    _swing_coverage(C, prev, T, sure & valid[:, None], st)

    # boxes: broken by a sure swing, kept where no swing can have touched them
    box_sure = np.zeros((N, C.B), dtype=bool)
    box_maybe = np.zeros((N, C.B), dtype=bool)
    if C.B:
        at_box = (T.kind == rr.BOX)[:, :, None] & (T.idx[:, :, None] == np.arange(C.B)[None, None, :])
        box_sure = (sure[:, :, None] & at_box).any(1)
        box_maybe = (maybe[:, :, None] & np.where(graze[:, :, None], prev.box_on[:, None, :], at_box)).any(1)
        kept = _same_boxes(prev, new)
        gone = prev.box_on & ~kept
        if C.damage >= C.box_health:
            st.add('box_breaks', (box_sure & valid[:, None]).sum())
            st.add('box_wrong', ((box_sure & kept) | (gone & ~box_sure & ~box_maybe))[valid].sum())
        # a broken box's item, due in the step before, is in this row unless somebody stands on it
        for n in np.nonzero(due & valid)[0]:
            for p in due_pos[n]:
                there = (new.bitems_on[n] & (new.bitems[n] == p).all(-1)).any()
                near = (alive1[n] & (np.sqrt(((new.pos[n] - p) ** 2).sum(-1)) < C.pickup_r + BAND)).any()
                st.add('box_items_due', 1)
                st.add('box_wrong', int(not there and not near))
        L.due = [[] for _ in range(N)]
        for n in np.nonzero(gone.any(-1))[0]:
            L.due[n] = [prev.box_pos[n, b].astype(np.float32).astype(np.float64) for b in np.nonzero(gone[n])[0]] if valid[n] else []

    # cooldowns
    if C.cooldown:
        st.add('cooldown_blocked', (pressed & hit_any & ~graze & (L.cd_lo > 0) & valid[:, None]).sum())
        fired = sure.copy()
        for n, i in zip(*np.nonzero(maybe & ~graze & valid[:, None])):
            # the only doubt is the cooldown: a foe or a box nobody else touched shows whether it fired
            j = int(T.idx[n, i])
            if T.kind[n, i] == rr.AGENT and foe[n, i, j] and both[n, j] and touched[n, :, j].sum() == 1 and not (zg[n, j] and not endgame[n]):
                if resid[n, j] == -C.damage:
                    fired[n, i] = True
                    st.add('resync_fired', 1)
                elif resid[n, j] == 0:
                    L.cd_lo[n, i] = max(L.cd_lo[n, i], 1)
                    maybe[n, i] = False
                else:
                    st.add('ledger_wrong', 1)
            elif T.kind[n, i] == rr.BOX and C.damage >= C.box_health and not box_sure[n, j] and not C.rc.box_ownership:
                # (an owned box stays when anybody but its owner hits it: it shows nothing about the cooldown)
                if (maybe[n, :] & ~graze[n, :] & (T.kind[n, :] == rr.BOX) & (T.idx[n, :] == j)).sum() == 1:
                    if gone[n, j]:
                        fired[n, i] = True
                        st.add('resync_fired', 1)
                    else:
                        L.cd_lo[n, i] = max(L.cd_lo[n, i], 1)
                        maybe[n, i] = False
        open_ = maybe & ~fired
        L.cd_lo = np.where(fired, C.cooldown, np.where(open_, np.where(~graze & hit_any, np.minimum(np.maximum(L.cd_lo, 1), C.cooldown), 0), L.cd_lo))
        L.cd_hi = np.where(fired | open_, C.cooldown, L.cd_hi)
        L.cd_lo, L.cd_hi = np.maximum(L.cd_lo - 1, 0), np.maximum(L.cd_hi - 1, 0)
    return SimpleNamespace(blind=placed | due, due_pos=due_pos, used_any=alive0 & (a[..., 4] == 1), gave=alive0 & (a[..., 5] == 1),
                           swings=swings)


def _near_rim(new, prev):
    d = new.pos - prev.zone[:, None, 0:2]
    return np.abs(np.sqrt((d * d).sum(-1)) - prev.zone[:, None, 2]) < RIM


def _swing_coverage(C, prev, T, sure, st):
    """Swings stopped by an item or a box with an agent behind it on the ray."""
    ang = prev.angle
    d = C.melee_range * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    fa, _ = pr.ray_circles(prev.pos, d, prev.pos[:, None], C.r, prev.present[:, None] & ~np.eye(C.A, dtype=bool)[None])
    behind = np.isfinite(fa).any(-1)
    st.add('swing_item_before_agent', (sure & behind & ((T.kind == rr.HEAL) | (T.kind == rr.BITEM))).sum())
    st.add('swing_box_before_agent', (sure & behind & (T.kind == rr.BOX)).sum())
    st.add('swing_blocked', (sure & behind & ((T.kind == rr.HEAL) | (T.kind == rr.BITEM) | (T.kind == rr.BOX))).sum())


# ---------------------------------------------------------------------------
# law D
# ---------------------------------------------------------------------------
def law_pickup(C, prev, new, valid, led, L, st, t):
    """Law D: a heal or box item farther than the pickup radius + BAND from
    every present agent's new position is still in the next row; one within
    radius - BAND of a present agent with room in its inventory is gone, and
    that agent's slot block shows the kind of the last item it took (box items
    are offered before heals, each kind in slot order, until the inventory is
    full).

    The law counts each agent's inventory from the reset on: `use` takes the
    top item off (before the pickup), every pickup adds one.  It stops judging
    the "gone" direction for an agent, until the episode ends, once the count
    is in doubt: an item within BAND of the radius, a `give` pressed anywhere in
    the env, an agent dying within reach (its items drop around it), or a box
    item due from a box broken the step before (law C's `blind` steps, for
    agents near the spot).  `give`, placing and DeathDrop themselves are
    judged by tests/items_laws.py, which keeps every stack item by item."""
    N, A = prev.N, C.A
    alive1 = new.present
    # uses come first
    L.depth = np.where(led.used_any & (L.depth > 0), L.depth - 1, L.depth)
    L.known &= ~led.gave.any(-1)[:, None]
    died = prev.present & ~new.present
    if died.any():
        d = prev.pos[:, :, None, :] - prev.pos[:, None, :, :]
        close = (np.sqrt((d * d).sum(-1)) < 2.0) & died[:, None, :] & ~(L.known & (L.depth == 0))[:, None, :]
        L.known &= ~close.any(-1)
    for n in np.nonzero(led.blind)[0]:
        for p in led.due_pos[n]:
            L.known[n] &= np.sqrt(((new.pos[n] - p) ** 2).sum(-1)) > C.pickup_r + 0.5
    ipos = np.concatenate([prev.bitems, prev.heals], axis=1)      # the order in which items are offered
    ion = np.concatenate([prev.bitems_on, prev.heals_on], axis=1)
    is_heal = np.concatenate([np.zeros(C.B, dtype=bool), np.ones(C.H, dtype=bool)])
    if ipos.shape[1] == 0:
        return
    inside, gz = rr.in_radius(ipos[:, None, :, :], new.pos[:, :, None, :], C.pickup_r, BAND)     # [N, A, I]
    cand = inside & ~gz & ion[:, None, :] & alive1[:, :, None]
    doubt = gz & ion[:, None, :] & alive1[:, :, None]
    still = np.concatenate([_same_items(prev.bitems, prev.bitems_on, new.bitems, new.bitems_on),
                            _same_items(prev.heals, prev.heals_on, new.heals, new.heals_on)], axis=1)
    far = ion & ~(cand | doubt).any(1) & valid[:, None]
    st.add('pickup_far', far.sum())
    st.add('pickup_wrong', (far & ~still).sum())
    room = C.slots - L.depth
    order = np.cumsum(cand, axis=-1)                               # 1-based rank among the agent's candidates
    ok = L.known & ~doubt.any(-1) & alive1 & valid[:, None]
    takes = cand & (order <= room[:, :, None]) & ok[:, :, None]
    n_take = takes.sum(-1)
    must_go = takes.any(1)
    st.add('pickups', must_go.sum())
    st.add('pickup_wrong', (must_go & still).sum())
    if (must_go & still).any() and 'pickup_wrong' not in st.where:
        st.where['pickup_wrong'] = (t,) + tuple(int(x[0]) for x in np.nonzero(must_go & still))
    last = (takes.shape[-1] - 1) - np.argmax(takes[..., ::-1], axis=-1)
    took = n_take > 0
    top_heal = is_heal[last]
    st.add('slot_wrong', (took & np.where(top_heal, ~new.heal_slot | new.box_slot, ~new.box_slot | new.heal_slot)).sum())
    L.depth = np.where(ok, L.depth + n_take, L.depth)
    L.known &= ~(doubt.any(-1) & alive1)
    # an inventory the law knows: empty shows no item, otherwise one of the two slots is filled
    sure = L.known & alive1 & valid[:, None]
    st.add('slot_wrong', (sure & ((L.depth > 0) != (new.heal_slot | new.box_slot))).sum())
    st.add('inventory_known', sure.sum())
    st.add('inventory_unknown', (~L.known & alive1 & valid[:, None]).sum())


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------
def _noise(rng, shape, p):
    return (rng.random(shape) < p).astype(np.int8)


def _standoff(rows, toward, point, dist):
    """the point `dist` beyond `point` as seen from `toward`"""
    d = point - toward
    n = np.sqrt((d * d).sum(-1, keepdims=True))
    return point + dist * d / np.maximum(n, 1e-9)


def drive_hide(t, rows, seeds, rng, C):
    """Alternately seek the far side of the nearest box from the nearest other
    agent, and turn on the spot (seek's constant turn, no thrust); attack
    pressed at random."""
    A = C.A
    others = rows.present[:, None, :] & ~np.eye(A, dtype=bool)[None]
    foe = pr.nearest(rows, rows.pos, others)
    box = pr.nearest(rows, rows.box_pos, rows.box_on)
    a = pr.seek(rows, _standoff(rows, foe, box, 1.3))
    if (t // 40) % 2:
        a[..., 0:2] = 1
    a[..., 3] = _noise(rng, a.shape[:2], 0.1) * rows.present   # now and then a box breaks and leaves its item
    return a


def drive_forage(t, rows, seeds, rng, C):
    """Seek the nearest heal or box item; use and attack pressed at random (a
    swing now and then breaks a box, whose item is then sought)."""
    pts = np.concatenate([rows.heals, rows.bitems], axis=1)
    on = np.concatenate([rows.heals_on, rows.bitems_on], axis=1)
    a = pr.seek(rows, pr.nearest(rows, pts, on))
    a[..., 3] = _noise(rng, a.shape[:2], 0.3)
    a[..., 4] = _noise(rng, a.shape[:2], 0.05)
    a[~rows.present] = (1, 1, 1, 0, 0, 0)
    return a


def drive_brawl(t, rows, seeds, rng, C):
    a = pr.duel(rows)
    a[..., 3] = 1
    # turn toward the foe instead of at a constant rate, so that swings land
    A = C.A
    on = (rows.alive & rows.present)[:, None, :] & ~np.eye(A, dtype=bool)[None]
    tg = pr.nearest(rows, rows.pos, on)
    d = pr._rot(-rows.angle, np.where(np.isfinite(tg), tg - rows.pos, 0.0))
    bearing = np.arctan2(d[..., 1], d[..., 0])
    a[..., 2] = 1 + np.sign(np.where(np.abs(bearing) < 0.05, 0.0, bearing)).astype(np.int8)
    a[~rows.present] = (1, 1, 1, 0, 0, 0)
    return a


def drive_zone(t, rows, seeds, rng, C):
    """Seek the point of the zone's rim nearest to the agent, alternately just
    inside and just outside it."""
    c, r = rows.zone[:, None, 0:2], rows.zone[:, None, 2:3]
    d = rows.pos - c
    n = np.sqrt((d * d).sum(-1, keepdims=True))
    u = np.where(n > 1e-6, d / np.maximum(n, 1e-6), np.array([1.0, 0.0]))
    side = np.where(((t // 15) + np.arange(C.A)) % 2 == 0, 0.15, -0.15)[None, :, None]
    return pr.seek(rows, c + (r + side) * u)


# the zone scenario keeps the stock radii, damage and random centres; its cooldown is 12 steps where the
# stock is 100, because the stock zone reaches its endgame at step 800, beyond every run here
ZONE_CFG = dict(C1_CONFIG, safe_zone={'phases': 5, 'cooldown': 12, 'damage': 1, 'radiuses': [10, 5, 2.5, 1],
                                      'centers': 'random'})
CONTINUOUS = {'range': 2, 'damage': 20, 'drift': True}


def scenario(name):
    s = {
        'hide': dict(cfg=C5_CONFIG, driver=drive_hide),
        'forage': dict(cfg=dict(C5_CONFIG, inventory={'slots': 2}), driver=drive_forage),
        'brawl_2v2': dict(cfg=C3_CONFIG, driver=drive_brawl),
        'brawl_ffa4': dict(cfg=dict(C5_CONFIG, melee=CONTINUOUS, inventory={'slots': 1}), driver=drive_brawl),
        'zone': dict(cfg=ZONE_CFG, driver=drive_zone),
    }[name]
    return SimpleNamespace(name=name, **s)


def twin_configs(cfg):
    """(omniscient, non-omniscient): the config with only the observation key set."""
    return dict(cfg, observation={'omniscent': True}), dict(cfg, observation={'omniscent': False})


SCENARIOS = ('hide', 'forage', 'brawl_2v2', 'brawl_ffa4', 'zone')

# Coverage floors: half of what the oracle reaches on the CPU test's seeds
# (8 seeds x 300 steps); both numbers are in profiles/rules_laws.txt.
FLOORS = {
    # the oracle: occ_box 3603, occ_agent 317, occ_item 1850, vis_seen 15552, out_of_cone_near 65674, mask0_others 746,
    # mask1_others 16830, mask0_heals 7483, mask1_heals 104396, mask0_boxes 5873, mask1_boxes 91395,
    # mask0_box_items 1455, mask1_box_items 13103
    'hide': {'occ_box': 1801, 'occ_agent': 158, 'occ_item': 925, 'vis_seen': 7776, 'out_of_cone_near': 32837,
        'mask0_others': 373, 'mask1_others': 8415, 'mask0_heals': 3741, 'mask1_heals': 52198, 'mask0_boxes': 2936,
        'mask1_boxes': 45697, 'mask0_box_items': 727, 'mask1_box_items': 6551},
    # the oracle: pickups 125, heal_uses 85, items_seen 6161, items_hidden 2528, cam_inside_item 4, box_breaks 50,
    # box_items_due 54
    'forage': {'pickups': 62, 'heal_uses': 42, 'items_seen': 3080, 'items_hidden': 1264, 'cam_inside_item': 2,
        'box_breaks': 25, 'box_items_due': 27},
    # the oracle: agent_hits 59, team_swings 58, cooldown_blocked 3884, box_breaks 6, deaths 24
    'brawl_2v2': {'agent_hits': 29, 'team_swings': 29, 'cooldown_blocked': 1942, 'box_breaks': 3, 'deaths': 12},
    # the oracle: agent_hits 197, box_breaks 30, swing_blocked 6, deaths 40
    'brawl_ffa4': {'agent_hits': 98, 'box_breaks': 15, 'swing_blocked': 3, 'deaths': 20},
    # the oracle: zone_out_rim 85, zone_in_rim 88, zone_endgame 729
    'zone': {'zone_out_rim': 42, 'zone_in_rim': 44, 'zone_endgame': 364},
}


def run(sc, reset, step, seeds, n_steps, record=None):
    """Drive N twin envs for n_steps with the scenario's controller, computed
    from the omniscient twin's rows, and apply the laws to every step.
    reset() -> (obs_omni, obs_non) [N, A, D]; step(actions) -> ((obs, rewards,
    done) of the omniscient twin, the same of the other), done envs already
    reset.  record(t, actions, non_twin_triple), if given, sees every step."""
    C = rr.constants(sc.cfg)
    st = Stats()
    rng = np.random.default_rng(4711 + len(sc.name))
    seeds = np.asarray(list(seeds))
    oo, on = reset()
    law_twins(C, (oo, None, None), (on, None, None), st)
    prev = rr.decode(oo, C)
    L = State(prev.N, C)
    law_visibility(C, prev, on, np.ones(prev.N, dtype=bool), st, -1)
    for t in range(n_steps):
        a = sc.driver(t, prev, seeds, rng, C)
        omni, non = step(a)
        if record is not None:
            record(t, a, non)
        law_twins(C, omni, non, st)
        done = np.asarray(omni[2], dtype=bool)
        new = rr.decode(omni[0], C)
        due = np.array([len(d) > 0 for d in L.due])
        law_visibility(C, new, non[0], done | (unchanged(prev, new) & ~due), st, t)
        led = law_ledger(C, prev, new, a, ~done, L, st, t)
        law_pickup(C, prev, new, ~done, led, L, st, t)
        L.reset(done)
        st.add('env_steps', (~done).sum())
        st.add('episodes', done.sum())
        prev = new
    return st


def check(sc, st):
    """The assertions both suites make on a finished run."""
    rep = st.report()
    c = st.count
    assert c['twin_diffs'] == 0, (sc.name, rep)
    assert c['vis_wrong'] == 0 and c['vis_phantom'] == 0, (sc.name, st.where.get('vis_wrong'), rep)
    assert c['vis_graze'] <= LIDAR_GRAZE_SHARE * c['vis_pairs'], (sc.name, rep)
    assert c['vis_skipped'] <= VIS_SKIP_SHARE * (c['vis_skipped'] + c['vis_judged_steps']), (sc.name, rep)
    assert c['ledger_wrong'] == 0 and c.get('box_wrong', 0) == 0, (sc.name, st.where.get('ledger_wrong'), rep)
    assert c['ledger_excluded'] <= LEDGER_SKIP_SHARE * c['ledger_steps'], (sc.name, rep)
    assert c.get('pickup_wrong', 0) == 0 and c.get('slot_wrong', 0) == 0, (sc.name, st.where.get('pickup_wrong'), rep)
    for k, floor in FLOORS[sc.name].items():
        assert c.get(k, 0) >= floor > 0, (sc.name, k, c.get(k, 0), floor, rep)
