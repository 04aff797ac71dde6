"""TEST INFRASTRUCTURE ONLY: the ledger of every item of an env and the laws
it must obey (the world a reset deals, placing a box, give, the tops of the
inventories, conservation, death drops, ownership), the scenarios that drive
envs into handing over, building and looting, and the loop that applies the one
to the other.  Shared by tests/test_items_reference.py (the C oracle, CPU) and
tests/test_gpu_items_laws.py (the HIP kernels).

The rows are omniscient, so nothing is hidden but the inventories below their
tops.  The ledger keeps those from each reset on: every agent's whole stack,
the items due from boxes broken in the last step, and per box shape its owner.
A box is followed by its 8 local vertices, bit for bit, through all its states:
box, due item, item on the ground, somebody's stack, a placed box (a box dealt
by the reset lists them in SetAsBox order, its item and every box placed from
it in hull order: items_ref.item_shape).

One env step, in the reference's order:

  1. due items spawn at the broken boxes' positions (Object.pre_step);
  2. use, in agent order: the top is popped, a heal heals, a box item places
     its box at pos + offset (cos angle, sin angle) (UseLast, ObjectItem.use);
  3. takers are computed for all agents from the poses before the step, then
     the gives run in agent order (GiveLast, Inventory.give);
  4. melee; 5. physics; 6. boxes whose health ran out break and their items
     become due; 7. cameras;
  8. agents whose health ran out are removed and drop their stack, bottom
     first, each item radius away at an angle drawn from the RNG (DeathDrop);
  9. pickup: every agent's query is made first, then each takes the items of
     its query in order, box items before heals, each in list order, while it
     has room.  An item in reach of two agents goes to both (the second `take`
     succeeds on the body the first one removed): the ledger counts the copy.

Every decision is exact but the two computed positions (laws F and J), whose
tolerances are measured.  A give or a pickup within BAND of its threshold and a
drop that may have been picked up as it landed make the stacks they touch
unknown until the episode ends; the shares are capped.

An env holds at most n_boxes boxes, n_boxes box items and n_heals heals, the
slots a row has: a due item, a placement or a drop beyond that is refused and
its item is gone (only the copies make more items than a reset deals).  The
ledger refuses in the engine's order and counts it (spawn_refused)."""
from __future__ import annotations

from collections import Counter
from types import SimpleNamespace

import numpy as np

import items_ref as ir
import physics_ref as pr
import rules_laws as rl
import rules_ref as rr
from masurvival.config import C3_CONFIG, C5_CONFIG
from physics_laws import LIDAR_GRAZE, LIDAR_GRAZE_SHARE, Stats, ulps

BAND = LIDAR_GRAZE
UNKNOWN_SHARE = 0.25      # agent-steps with an unknown stack, of the present agent-steps
UNJUDGED_SHARE = 0.40     # env-steps on which conservation cannot be judged
NOBODY, DOUBT = 'nobody', 'doubt'
HEAL_ITEM = (rr.HEAL, None, None)

# Position tolerances in fp32 ulps of the coordinate: 4 x the worst deviation of the
# unmodified oracle over the CPU scenarios (profiles/items_laws.txt).
TOL = {
    'place_pos': 2.36,     # oracle worst 0.5894
    'drop_radius': 4.0,    # oracle worst 0.9985
}


class Ledger:
    """What the laws carry from step to step, per env."""

    def __init__(self, N, C):
        self.N, self.A = N, C.A
        self.stack = [[[] for _ in range(C.A)] for _ in range(N)]   # (kind, 8 fp32 bit patterns, owner), bottom first
        self.known = np.ones((N, C.A), dtype=bool)
        self.due = [[] for _ in range(N)]                           # (position, bits), in the order the boxes broke
        self.owner = [{} for _ in range(N)]                         # bits -> agent index or team, or DOUBT
        self.unique = np.ones(N, dtype=bool)                        # the env's box shapes are pairwise distinct
        self.placed_before = [set() for _ in range(N)]
        self.refused_envs = set()                                   # envs in which a spawn was refused, ever
        self.breaker = [{} for _ in range(N)]                       # bits -> the agent whose swing set the owner
        self.rules = rl.State(N, C)                                 # law C's cooldown intervals

    def reset(self, envs, rows):
        self.rules.reset(envs)
        self.known[envs] = True
        for n in np.nonzero(envs)[0]:
            self.stack[n] = [[] for _ in range(self.A)]
            self.due[n], self.owner[n], self.placed_before[n], self.breaker[n] = [], {}, set(), {}
            shapes = {tuple(b) for b in rows.box_bits[n][rows.box_on[n]].tolist()}
            self.unique[n] = len(shapes) == int(rows.box_on[n].sum())


def _bits(row):
    return tuple(int(x) for x in row)


class _tuples:
    """[N, K, 8] -> per env, on demand, a list of K tuples"""

    def __init__(self, bits):
        self.bits, self.rows = bits, {}

    def __getitem__(self, n):
        if n not in self.rows:
            self.rows[n] = [tuple(r) for r in self.bits[n].tolist()]
        return self.rows[n]


def _dev(st, key, value, where):
    st.worst.setdefault(key, 0.0)
    if value > st.worst[key]:
        st.worst[key], st.where[key] = float(value), where


def _first(st, key, where):
    st.add(key, 1)
    st.where.setdefault(key, where)


# ---------------------------------------------------------------------------
# law E
# ---------------------------------------------------------------------------
def law_reset(C, rows, envs, st):
    """Law E: in a reset row every agent, heal and box stands on a cell centre
    of the spawn grid, no two on one; every box is a centred rectangle in
    SetAsBox order, at least min_w x min_h, of box_size where shapes are not
    randomised, at angle 0; every health is full, every inventory slot empty,
    and the zone is the first configured circle."""
    envs = np.asarray(envs, dtype=bool)
    if not envs.any():
        return
    cells = ir.spawn_cells(C).astype(np.float32).astype(np.float64)
    pos = np.concatenate([rows.pos, rows.heals, rows.box_pos], axis=1)[envs]
    on = np.concatenate([rows.present, rows.heals_on, rows.box_on], axis=1)[envs]
    bad = (~on).sum()                                        # everything is there
    hit = (pos[:, :, None, :] == cells[None, None]).all(-1)  # [n, M, cells]
    bad += (on & (hit.sum(-1) != 1)).sum()
    bad += ((hit & on[..., None]).sum(1) > 1).sum()          # two bodies on one cell
    w, h, ok = ir.rect_dims(rows.box_local[envs])
    lo = 1.0 - 2.0 ** -23                                    # the half extents are fp32: twice a rounded half
    bad += (~ok | (w < C.min_w * lo) | (h < C.min_h * lo) | (rows.box_angle[envs] != 0)).sum()
    if not C.randomized:
        bad += ((w != C.box_size) | (h != C.box_size)).sum()
    bad += (rows.health[envs] != C.full_health).sum()
    bad += (rows.slot_raw[envs] != 1).sum() + (rows.heal_amount[envs] != 0).sum() + (rows.top_bits[envs] != 0).sum()
    bad += (~rows.bitems_on[envs]).sum() != rows.bitems_on[envs].size
    z = rows.zone[envs]
    bad += (z[:, 2] != C.zone_r0).sum()
    centers = C.rc.config['safe_zone']['centers']
    if isinstance(centers, str):
        bad += (np.abs(z[:, 0:2]) > (C.floor - 2 * C.zone_r0) / 2.0).sum()
    else:
        bad += (z[:, 0:2] != np.asarray(centers[0], dtype=np.float32).astype(np.float64)).sum()
    st.add('reset_rows', envs.sum())
    st.add('reset_wrong', bad)
    st.add('reset_shapes_clash', (envs & ~_unique(rows)).sum())


def _unique(rows):
    out = np.ones(rows.N, dtype=bool)
    for n in range(rows.N):
        b = rows.box_bits[n][rows.box_on[n]]
        out[n] = len({tuple(x) for x in b.tolist()}) == len(b)
    return out


# ---------------------------------------------------------------------------
# law H
# ---------------------------------------------------------------------------
def law_tops(C, rows, L, valid, st, t):
    """Law H: for every present agent whose stack the ledger knows, the two
    slot masks show the kind of its top (both 1 when it is empty), heal_slot
    the healing and box_slot the top's 8 vertex floats bit for bit.  An agent
    that fails is counted once and then unknown."""
    judged = rows.present & L.known & valid[:, None]
    st.add('tops_judged', judged.sum())
    for n, i in zip(*np.nonzero(judged)):
        s = L.stack[n][i]
        hm, bm = rows.slot_raw[n, i]
        if not s:
            ok = hm == 1 and bm == 1 and rows.heal_amount[n, i] == 0 and not rows.top_bits[n, i].any()
        elif s[-1][0] == rr.HEAL:
            ok = hm == 0 and bm == 1 and rows.heal_amount[n, i] == C.healing and not rows.top_bits[n, i].any()
        else:
            ok = hm == 1 and bm == 0 and rows.heal_amount[n, i] == 0 and _bits(rows.top_bits[n, i]) == s[-1][1]
        if not ok:
            _first(st, 'top_wrong', (t, int(n), int(i)))
            L.known[n, i] = False


# ---------------------------------------------------------------------------
# laws F, G, I, J, K: one pass over the step's events
# ---------------------------------------------------------------------------
def law_items(C, prev, new, actions, valid, led, L, st, t):
    """Laws F (placing), G (give), I (conservation), J (death drops) and K
    (ownership) on one step: the ledger replays the step's events in the
    reference's order and compares what it predicts with the new row.  Law G
    has no check of its own: a wrong give shows in the tops (law H) and in the
    conservation (law I)."""
    N, A = prev.N, C.A
    a = np.asarray(actions)
    alive0, alive1 = prev.present, new.present
    use_p = alive0 & (a[..., 4] == 1)
    give_p = alive0 & (a[..., 5] == 1)
    spot = ir.placement(prev.pos, prev.angle, C.offset)
    kept = rl._same_boxes(prev, new)
    gone = prev.box_on & ~kept
    fresh_box = new.box_on & ~rl._same_boxes(new, prev)
    died = alive0 & ~alive1
    sw = led.swings

    # the bodies GiveLast finds that no row shows: boxes placed by this step's uses and the due items
    # An env holds at most n_boxes boxes, n_boxes box items and n_heals heals, the slots a row has; a spawn
    # beyond that is refused and the item is gone (only the copies of double pickups make more than a reset deals).
    # Due items come first, in the order their boxes broke; then the placements, in agent order.
    over = {}
    for n in np.nonzero(valid)[0]:
        room = C.B - int(prev.bitems_on[n].sum())
        if len(L.due[n]) > room:
            over[n], L.due[n] = [b for _, b in L.due[n][room:]], L.due[n][:room]
    placing = use_p & prev.box_slot
    refused = placing & (prev.box_on.sum(-1)[:, None] + np.cumsum(placing, axis=1) > C.B)
    placing = placing & ~refused
    nd = max([len(d) for d in L.due] + [0])
    X = SimpleNamespace(
        pos=np.concatenate([spot, np.zeros((N, nd, 2))], axis=1), on=np.concatenate([placing, np.zeros((N, nd), dtype=bool)], axis=1),
        kind=np.concatenate([np.full((N, A), ir.PLACED), np.full((N, nd), ir.DUE)], axis=1),
        idx=np.concatenate([np.broadcast_to(np.arange(A), (N, A)), np.broadcast_to(np.arange(nd), (N, nd))], axis=1).copy())
    for n in range(N):
        for k, (p, _) in enumerate(L.due[n]):
            X.pos[n, A + k], X.on[n, A + k] = p, True
    Tk = ir.give_taker(prev, C, X, BAND)

    # pickup geometry against the items of the previous row (box items, then heals)
    ipos = np.concatenate([prev.bitems, prev.heals], axis=1)
    ion = np.concatenate([prev.bitems_on, prev.heals_on], axis=1)
    inside, gz = rr.in_radius(ipos[:, None, :, :], new.pos[:, :, None, :], C.pickup_r, BAND)
    cand = inside & ~gz & ion[:, None, :] & alive1[:, :, None]
    doubt = gz & ion[:, None, :] & alive1[:, :, None]
    if died.any():
        body, free = ir.corpse(prev, C, a, new)
        far = ir.max_step(prev, C, a)

    # the shapes as tuples of 8 bit patterns: boxes (in their items' vertex order), items on the ground
    shape0, shape1 = _tuples(prev.box_item_bits), _tuples(new.box_item_bits)
    ishape0, ishape1 = _tuples(prev.bitem_bits), _tuples(new.bitem_bits)
    raw1 = _tuples(new.box_bits)
    if C.B:
        at = (sw.T.kind == rr.BOX)[:, :, None] & (sw.T.idx[:, :, None] == np.arange(C.B)[None, None, :])
        swung = ((sw.sure | sw.maybe)[:, :, None] & at).any(1) | (sw.maybe & sw.graze).any(-1)[:, None]
    else:
        swung = gone
    # an env-step in which nothing can happen to an item: nothing may have changed
    has_due = np.array([len(d) > 0 for d in L.due])
    quiet = ~(np.isin(np.arange(N), list(over)) | use_p.any(-1) | give_p.any(-1) | died.any(-1) | gone.any(-1) | swung.any(-1) | has_due | cand.any((1, 2)) | doubt.any((1, 2)))
    same = rl.unchanged(prev, new)
    st.add('agent_steps', ((alive0 | alive1) & valid[:, None]).sum())
    st.add('shared_reach', ((cand.sum(1) > 1) & valid[:, None]).sum())     # items of the previous row in reach of two agents
    for n in np.nonzero(valid)[0]:
        stack, known = L.stack[n], L.known[n]
        judge = bool(known[alive0[n] | alive1[n]].all())            # law I needs every present stack
        if quiet[n]:
            st.add('conserve_steps' if judge else 'conserve_skipped', 1)
            if judge and not same[n]:
                _first(st, 'conserve_wrong', (t, int(n)))
            continue
        box_before = Counter(shape0[n][b] for b in np.nonzero(prev.box_on[n])[0])
        box_before.update(ishape0[n][k] for k in np.nonzero(prev.bitems_on[n])[0])
        box_before.update(b for _, b in L.due[n])
        box_before.update(over.get(n, ()))
        box_before.update(it[1] for s in stack for it in s if it[0] == rr.BITEM)
        heals_before = int(prev.heals_on[n].sum()) + sum(it[0] == rr.HEAL for s in stack for it in s)
        lost_box, lost_heal, used_heal = Counter(over.get(n, ())), 0, 0
        st.add('spawn_refused', len(over.get(n, ())))
        if n in over:
            L.refused_envs.add(int(n))

        # 2. use
        placed = []
        for i in np.nonzero(use_p[n])[0]:
            if not known[i]:
                continue
            if stack[i]:
                kind, bits, _ = stack[i].pop()
                if kind == rr.HEAL:
                    used_heal += 1
                elif refused[n, i]:
                    lost_box[bits] += 1              # the item is used up and no box appears
                    st.add('spawn_refused', 1)
                    L.refused_envs.add(int(n))
                else:
                    placed.append((i, bits))
        # law F
        for i, bits in placed:
            want = spot[n, i]
            best = np.inf
            for b in np.nonzero(fresh_box[n])[0]:
                if raw1[n][b] == bits and new.box_angle[n, b] == 0:
                    best = min(best, float(ulps(np.abs(new.box_pos[n, b] - want).max(), np.abs(want).max())))
            st.add('placements', 1)
            if not np.isfinite(best):
                _first(st, 'place_wrong', (t, int(n), int(i)))
            else:
                _dev(st, 'place_pos', best, (t, int(n), int(i)))
            st.add('place_q%d' % (int(np.floor(np.mod(prev.angle[n, i], 2 * np.pi) / (np.pi / 2))) % 4), 1)
            if a[n, i, 3] == 1 and sw.ready[n, i] and sw.T.kind[n, i] == rr.NONE:
                st.add('placed_hit', 1)              # nothing else was in the swing's way: it struck the new box, which stays
            if L.unique[n]:
                st.add('replaced', bits in L.placed_before[n])
                L.placed_before[n].add(bits)

        # 3. give
        got = set()
        for i in np.nonzero(give_p[n])[0]:
            if known[i] and not stack[i]:
                continue
            kind, j = int(Tk.kind[n, i]), int(Tk.idx[n, i])
            st.add('give_events', 1)
            if Tk.graze[n, i]:
                st.add('give_graze', 1)
                known[i] = False
                known[Tk.reach[n, i]] = False
                continue
            if kind != rr.AGENT:
                st.add('give_to_' + {rr.NONE: 'nobody', rr.HEAL: 'heal', rr.BOX: 'box', rr.BITEM: 'box_item', rr.WALL: 'wall',
                                     ir.PLACED: 'placed', ir.DUE: 'due'}[kind], 1)
                st.add('give_to_non_agent', 1)
                continue
            st.add('give_to_agent', 1)
            if prev.team[n, i] != prev.team[n, j] and C.teams:
                st.add('give_refused', 1)
                continue
            if not known[i]:
                known[j] = False
                continue
            item = stack[i].pop()
            if i in got:
                st.add('give_two_hands', 1)
            if not known[j]:
                judge = False                        # the item went into a stack nobody counts
                continue
            if len(stack[j]) < C.slots:
                stack[j].append(item)
                got.add(j)
                st.add('give_taken', 1)
            else:
                st.add('give_lost', 1)
                if item[0] == rr.HEAL:
                    lost_heal += 1
                else:
                    lost_box[item[1]] += 1

        # 4 - 6. swings at boxes: ownership (law K), and no box goes unless somebody can have hit it
        _law_owner(C, prev, n, kept[n], gone[n], swung[n], shape0[n], sw, L, st, t)
        due_new = [(prev.box_pos[n, b].astype(np.float32).astype(np.float64), shape0[n][b]) for b in np.nonzero(gone[n])[0]]

        # 8. deaths
        ground = [(rr.BITEM, ishape0[n][k], k) for k in np.nonzero(prev.bitems_on[n])[0]]
        due_items = [(rr.BITEM, b, p) for p, b in L.due[n]]
        heals = [(rr.HEAL, None, C.B + k) for k in np.nonzero(prev.heals_on[n])[0]]
        drops, dead, dead_unknown = [], [], False
        for i in np.nonzero(died[n])[0]:
            if known[i]:
                if stack[i]:
                    dead.append(i)
                    drops += [(it[0], it[1]) for it in stack[i]]
                    st.add('deaths_depth%s' % ('3p' if len(stack[i]) >= 3 else len(stack[i])), 1)
                else:
                    st.add('deaths_depth0', 1)
            else:
                judge, dead_unknown = False, True
                dead.append(i)
            stack[i] = []
        if not dead_unknown:
            # the drops land in order while there is room for their kind
            nh, ni, landing = int(prev.heals_on[n].sum()), len(ground) + len(due_items), []
            for kind, bits in drops:
                if kind == rr.HEAL and nh < C.H:
                    nh, landing = nh + 1, landing + [(kind, bits)]
                elif kind == rr.BITEM and ni < C.B:
                    ni, landing = ni + 1, landing + [(kind, bits)]
                else:
                    st.add('spawn_refused', 1)
                    L.refused_envs.add(int(n))
                    if kind == rr.HEAL:
                        lost_heal += 1
                    else:
                        lost_box[bits] += 1
            drops = landing
        # who could reach a drop as it lands
        finder = np.zeros(A, dtype=bool)
        for i in dead:
            c, reach = (body[n, i], 0.0) if free[n, i] else (prev.pos[n, i], far[n])
            d = new.pos[n] - c
            finder |= alive1[n] & (np.sqrt((d * d).sum(-1)) < C.pickup_r + C.drop_r + reach + BAND)

        # 9. pickup
        taken = Counter()
        takes = {}
        for i in np.nonzero(alive1[n])[0]:
            if doubt[n, i].any() or any(rr.in_radius(new.pos[n, i], p, C.pickup_r, BAND)[1] for _, _, p in due_items):
                if known[i]:
                    st.add('pickup_graze', 1)
                known[i] = False
            if not known[i]:
                if cand[n, i].any() or doubt[n, i].any() or any(rr.in_radius(new.pos[n, i], p, C.pickup_r + BAND)[0] for _, _, p in due_items):
                    judge = False                    # it may have taken any of them
                continue
            mine = [g for g in ground if cand[n, i, g[2]]]
            mine += [g for g in due_items if rr.in_radius(new.pos[n, i], g[2], C.pickup_r, BAND)[0]]
            mine += [h for h in heals if cand[n, i, h[2]]]
            takes[i] = mine[:C.slots - len(stack[i])]
            for it in takes[i]:
                taken[(it[0], it[1], id(it))] += 1
        copies_box, copies_heal = Counter(), 0
        for (kind, bits, _), c in taken.items():
            st.add('pickups', 1)
            if c > 1:
                st.add('double_pickups', c - 1)
                if kind == rr.HEAL:
                    copies_heal += c - 1
                else:
                    copies_box[bits] += c - 1
        for i, mine in takes.items():
            stack[i] += [(it[0], it[1], L.owner[n].get(it[1])) for it in mine]

        # what should lie on the ground now, but for the drops
        stay_box = Counter(it[1] for it in ground + due_items if taken[(it[0], it[1], id(it))] == 0)
        stay_heal = sum(taken[(h[0], h[1], id(h))] == 0 for h in heals)
        now_box = Counter(ishape1[n][k] for k in np.nonzero(new.bitems_on[n])[0])
        now_heal = int(new.heals_on[n].sum())
        extra_box, extra_heal = now_box - stay_box, now_heal - stay_heal
        want_box = Counter(b for k, b in drops if k == rr.BITEM)
        want_heal = sum(k == rr.HEAL for k, _ in drops)
        landed = extra_box == want_box and extra_heal == want_heal and not (stay_box - now_box)
        if dead_unknown:
            known[finder] = False
        elif dead:
            st.add('drop_events', len(dead))
            # a finder can have taken a drop only with a slot left before the heals it took (box items come first)
            able = [i for i in np.nonzero(finder)[0] if not known[i] or
                    len(stack[i]) - sum(it[0] == rr.HEAL for it in takes.get(i, ())) < C.slots]
            if not landed and able:
                # an item short, somebody in reach: picked up as it landed.  The finder's stack is unknown from here on.
                st.add('drop_found', 1)
                known[finder] = False
                judge = False
            elif landed and judge:
                st.add('drop_box_items', sum(want_box.values()))
                _law_drops(C, prev, new, n, dead, body, free, far, [p for p, _ in L.due[n]], st, t)

        # law I
        if judge:
            st.add('conserve_steps', 1)
            box_after = Counter(shape1[n][b] for b in np.nonzero(new.box_on[n])[0]) + now_box
            box_after.update(b for _, b in due_new)
            box_after.update(it[1] for i in np.nonzero(alive1[n])[0] for it in stack[i] if it[0] == rr.BITEM)
            heals_after = now_heal + sum(it[0] == rr.HEAL for i in np.nonzero(alive1[n])[0] for it in stack[i])
            if box_after != box_before - lost_box + copies_box or heals_after != heals_before - used_heal - lost_heal + copies_heal:
                _first(st, 'conserve_wrong', (t, int(n)))
            st.add('heals_used', used_heal)
        else:
            st.add('conserve_skipped', 1)
        L.due[n] = due_new
    for n in np.nonzero(~valid)[0]:
        L.due[n] = []
    st.add('unknown_steps', (~L.known & alive1 & valid[:, None]).sum())


def _law_drops(C, prev, new, n, dead, body, free, far, due_pos, st, t):
    """Law J, the positions: every item that is new on the ground lies
    death_drop.radius from the body of a dying agent that was in free flight,
    or within radius + the step's largest displacement of where a dying agent
    in contact stood."""
    old_b = {tuple(p) for p in prev.bitems[n][prev.bitems_on[n]].tolist()}
    old_h = {tuple(p) for p in prev.heals[n][prev.heals_on[n]].tolist()}
    new_pts = [p for p in new.bitems[n][new.bitems_on[n]] if tuple(p.tolist()) not in old_b]
    new_pts += [p for p in new.heals[n][new.heals_on[n]] if tuple(p.tolist()) not in old_h]
    all_free = all(free[n, i] for i in dead)
    for p in new_pts:
        if any((p == q).all() for q in due_pos):
            continue                                   # a due item at its box's place, not a drop
        if all_free:
            dev = min(float(ulps(abs(np.sqrt(((p - body[n, i]) ** 2).sum()) - C.drop_r), np.abs(body[n, i]).max())) for i in dead)
            st.add('drops_free', 1)
            _dev(st, 'drop_radius', dev, (t, int(n)))
        else:
            d = min(float(np.sqrt(((p - prev.pos[n, i]) ** 2).sum())) for i in dead)
            st.add('drops_contact', 1)
            if d > C.drop_r + far[n] + BAND:
                _first(st, 'drop_wrong', (t, int(n)))


def _law_owner(C, prev, n, kept, gone, swung, shapes, sw, L, st, t):
    """Law K.  A sure swing (law C's: attack pressed, a closest hit beyond
    doubt, off cooldown) at a box of the previous row breaks it if its shape
    has no owner yet or the hitter is the owner (its team, with teams); a swing
    by anybody else leaves it; the first break sets the owner.  Without
    ownership every sure swing breaks.  A box nobody can have hit stays."""
    T = sw.T
    owner = L.owner[n]
    for b in np.nonzero(prev.box_on[n] & (gone | swung))[0]:
        at = (T.kind[n] == rr.BOX) & (T.idx[n] == b)
        sure = np.nonzero(sw.sure[n] & at)[0]
        maybe = bool((sw.maybe[n] & (sw.graze[n] | at)).any())
        if gone[b] and not len(sure) and not maybe:
            _first(st, 'box_vanished', (t, int(n), int(b)))
        if C.damage < C.box_health:
            continue
        bits = shapes[b]
        own = owner.get(bits, NOBODY) if C.ownership else NOBODY
        ids = [int(prev.team[n, i]) if C.teams else int(i) for i in sure]
        judged = C.ownership and L.unique[n] or not C.ownership
        if len(sure) and not maybe and own != DOUBT and judged:
            if own == NOBODY or own in ids:
                st.add('owner_breaks' if own != NOBODY else 'free_breaks', 1)
                if own != NOBODY and C.teams and L.breaker[n].get(bits) not in [int(i) for i in sure]:
                    st.add('mate_breaks', 1)         # the badge owns it, not the agent that broke it first
                if kept[b]:
                    _first(st, 'owner_wrong', (t, int(n), int(b)))
            else:
                st.add('stranger_swings', 1)
                if gone[b]:
                    _first(st, 'owner_wrong', (t, int(n), int(b)))
        elif len(sure) and C.ownership:
            st.add('owner_unjudged', 1)
        if gone[b] and C.ownership and own == NOBODY:
            owner[bits] = ids[0] if len(sure) and not maybe and len(set(ids)) == 1 else DOUBT
            L.breaker[n][bits] = int(sure[0]) if len(sure) == 1 else None


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------
def _items(rows):
    return np.concatenate([rows.heals, rows.bitems], axis=1), np.concatenate([rows.heals_on, rows.bitems_on], axis=1)


def _holds(rows):
    return rows.heal_slot | rows.box_slot


def _clear_give(rows, C, kinds, margin=0.15):
    """[N, A]: the taker (without this step's placed boxes) is of one of `kinds`
    and well inside the radius, and no other body's distance is near its own."""
    T = ir.give_taker(rows, C, None, margin)
    return ~T.graze & np.isin(T.kind, kinds), T


def _turn_to(rows, a, heading):
    d = np.mod(heading - rows.angle + np.pi, 2 * np.pi) - np.pi
    a[..., 2] = 1 + np.sign(np.where(np.abs(d) < 0.1, 0.0, d)).astype(np.int8)


def drive_handover_2v2(t, rows, seeds, rng, C):
    """Forage (attack at random breaks boxes), then walk to the nearest
    teammate and give; every third phase walk to the nearest enemy and give."""
    A = C.A
    phase, k = divmod(t, 100)
    pts, on = _items(rows)
    tg = pr.nearest(rows, pts, on)
    tg = np.where(np.isfinite(tg), tg, pr.nearest(rows, rows.box_pos, rows.box_on))
    a = pr.seek(rows, tg)
    _face(rows, a, tg)
    a[..., 3] = rl._noise(rng, a.shape[:2], 0.5)
    if k >= 60:
        same = rows.team[:, :, None] == rows.team[:, None, :]
        who = (same if phase % 3 != 2 else ~same) & rows.present[:, None, :] & ~np.eye(A, dtype=bool)[None]
        a = pr.seek(rows, pr.nearest(rows, rows.pos, who))
        ok, _ = _clear_give(rows, C, [rr.AGENT])
        a[..., 5] = ok & _holds(rows)
    a[~rows.present] = (1, 1, 1, 0, 0, 0)
    return a


def _face(rows, a, tg):
    d = pr._rot(-rows.angle, np.where(np.isfinite(tg), tg - rows.pos, 0.0))
    bearing = np.arctan2(d[..., 1], d[..., 0])
    a[..., 2] = 1 + np.sign(np.where(np.abs(bearing) < 0.05, 0.0, bearing)).astype(np.int8)


THIN = 0.5     # a box this thin lets two agents at its two long sides both come near its centre


def _squeeze(t, rows, C, a):
    """Agents 0 and 1 of every env that has a box thinner than THIN, in cycles
    of 100 steps: empty the inventory, walk to the two long sides of the env's
    thinnest box, press against it facing its centre, break it at step 80 and
    keep pressing.  The box's item appears at its centre one step later, the
    two close in on it from rest at the same pace, and it comes within the
    pickup radius of both in the same step: the one way for two agent bodies,
    which cannot overlap, to have one item in reach together."""
    k = t % 100
    if C.B == 0 or k >= 95:
        return
    N = rows.N
    w, h, _ = ir.rect_dims(rows.box_local)
    thin = np.where(rows.box_on, np.minimum(w, h), np.inf)
    b = thin.argmin(-1)
    e = np.arange(N)
    width = thin[e, b]
    centre = rows.box_pos[e, b]
    normal = np.where((w[e, b] < h[e, b])[:, None], np.array([1.0, 0.0]), np.array([0.0, 1.0]))
    go = (width < THIN) & rows.present[:, 0] & rows.present[:, 1]
    if k > 80:       # the box is gone: its item lies where it stood
        two = SimpleNamespace(pos=rows.pos[:, :2])
        tg = pr.nearest(two, rows.bitems, rows.bitems_on)
        go = rows.present[:, 0] & rows.present[:, 1] & np.isfinite(tg).all((-1, -2))
    else:
        side = np.sign(((rows.pos[:, :2] - centre[:, None, :]) * normal[:, None, :]).sum(-1))
        side = np.where(side == 0, 1.0, side)
        side[:, 1] = np.where(side[:, 1] == side[:, 0], -side[:, 0], side[:, 1])     # the side it is on; agent 1 goes round if both are on one
        stand = centre[:, None, :] + side[..., None] * normal[:, None, :] * (width[:, None, None] / 2 + 0.9)
        tg = np.where(k < 60, stand, np.broadcast_to(centre[:, None, :], stand.shape))
    two = SimpleNamespace(pos=rows.pos[:, :2], angle=rows.angle[:, :2], alive=rows.alive[:, :2])
    act = pr.seek(two, tg)
    _face(two, act, tg)
    act[..., 3] = k == 80
    act[..., 4] = (k < 10) & (rows.heal_slot | rows.box_slot)[:, :2]
    a[:, :2] = np.where(go[:, None, None], act, a[:, :2])


def drive_handover_ffa4(t, rows, seeds, rng, C):
    """Forage with two slots; with something in hand press give wherever the
    taker is beyond doubt (another agent, a heal, a box, a box item), and now
    and then use and give in one step, so that the box just placed is the
    taker.  Agents 0 and 1 squeeze a thin box where the env has one."""
    pts, on = _items(rows)
    a = pr.seek(rows, pr.nearest(rows, pts, on))
    a[..., 3] = rl._noise(rng, a.shape[:2], 0.3)
    ok, T = _clear_give(rows, C, [rr.AGENT, rr.HEAL, rr.BOX, rr.BITEM])
    a[..., 5] = ok & _holds(rows) & (rl._noise(rng, a.shape[:2], 0.5) == 1) & (t % 50 >= 20)
    both = rows.box_slot & (rl._noise(rng, a.shape[:2], 0.3) == 1) & (T.dist > C.offset + 0.15)
    a[..., 4] = both | ((t % 20 == 0) & rows.heal_slot)
    a[..., 5] |= both
    _squeeze(t, rows, C, a)
    a[~rows.present] = (1, 1, 1, 0, 0, 0)
    return a


def drive_builder(t, rows, seeds, rng, C):
    """In cycles of 60 steps: walk to the nearest box item, or box if there is
    none, facing it, with attack pressed on even cycles (boxes break, their
    items are collected); stand and turn to a heading that depends on the
    agent, the env and the cycle; all place in one step, on odd cycles with
    attack pressed in that same step; then walk to the box nearest to another
    agent (which one turns with the cycle), most often the one it placed, and
    swing."""
    cycle, k = divmod(t, 60)
    if k < 25:
        tg = pr.nearest(rows, rows.bitems, rows.bitems_on)
        tg = np.where(np.isfinite(tg), tg, pr.nearest(rows, rows.box_pos, rows.box_on))
        a = pr.seek(rows, tg)
        _face(rows, a, tg)
        a[..., 3] = cycle % 2 == 0
    elif k < 40:
        a = pr.seek(rows, np.full(rows.pos.shape, np.nan))
        _turn_to(rows, a, (np.arange(C.A)[None, :] + cycle + (np.asarray(seeds) % 4)[:, None]) * (np.pi / 2) + 0.3)
        a[..., 4] = (k == 39) & rows.box_slot
        a[..., 3] = (k == 39) & (cycle % 2 == 1)
    else:
        whose = (np.arange(C.A) + 1 + cycle) % C.A                # the box nearest to another agent, in turn: often its own
        there = SimpleNamespace(pos=np.where(rows.present[:, whose, None], rows.pos[:, whose], rows.pos))
        tg = pr.nearest(there, rows.box_pos, rows.box_on)
        a = pr.seek(rows, tg)
        _face(rows, a, tg)
        a[..., 3] = 1
    a[~rows.present] = (1, 1, 1, 0, 0, 0)
    return a


def drive_loot(t, rows, seeds, rng, C):
    """Forage for 90 steps of every 200 (attack at random: boxes break), then brawl."""
    if t % 200 < 90:
        pts, on = _items(rows)
        a = pr.seek(rows, pr.nearest(rows, pts, on))
        a[..., 3] = rl._noise(rng, a.shape[:2], 0.3) * (rows.box_on.sum(-1) > C.B - 6)[:, None]
        a[~rows.present] = (1, 1, 1, 0, 0, 0)
        return a
    return rl.drive_brawl(t, rows, seeds, rng, C)


def drive_loot_zone(t, rows, seeds, rng, C):
    """Forage without a swing while the zone closes: agents die of the zone in free flight."""
    pts, on = _items(rows)
    a = pr.seek(rows, pr.nearest(rows, pts, on))
    a[~rows.present] = (1, 1, 1, 0, 0, 0)
    return a


def _c5(**kw):
    return dict(C5_CONFIG, **kw)


OWNED = dict(C5_CONFIG['boxes'], ownership=True)
LOOT_ZONE = dict(rl.ZONE_CFG['safe_zone'], damage=4)


# The `ffal` class at its limits: 8 slots, 24 heals, 16 owned boxes; a copy of test_gpu_capacity.TEAMS_BIG
# (test_gpu_items_laws asserts the two are equal), so that the CPU suite imports no GPU test module.
TEAMS_BIG = {
    'agents': {'n_agents': 4, 'agent_size': 1}, 'teams': {'twoteams': True},
    'spawn_grid': {'grid_size': 8, 'floor_size': 20},
    'heals': {'reset_spawns': {'n_items': 24, 'item_size': 0.5}, 'heal': {'healing': 50}},
    'boxes': {'reset_spawns': {'n_boxes': 16, 'box_size': 1}, 'ownership': True,
              'item': {'item_size': 0.5, 'offset': 0.75}, 'health': 20},
    'inventory': {'slots': 8},
    'safe_zone': {'phases': 5, 'cooldown': 25, 'damage': 4, 'radiuses': [10, 5, 2.5, 1], 'centers': 'random'},
    'melee': {'range': 2, 'damage': 20, 'cooldown': 40, 'drift': True}}


def scenario(name):
    if name == 'loot_ffal':
        return SimpleNamespace(name=name, cfg=TEAMS_BIG, driver=drive_loot)
    s = {
        'handover_2v2': dict(cfg=dict(C3_CONFIG, inventory={'slots': 2}), driver=drive_handover_2v2),
        'handover_ffa4': dict(cfg=_c5(inventory={'slots': 2}), driver=drive_handover_ffa4),
        'builder': dict(cfg=_c5(boxes=OWNED), driver=drive_builder),
        'builder_2v2': dict(cfg=_c5(boxes=OWNED, teams={'twoteams': True}, melee=rl.CONTINUOUS), driver=drive_builder),
        'loot': dict(cfg=_c5(melee=rl.CONTINUOUS, inventory={'slots': 4}, death_drop={'radius': 1.0}), driver=drive_loot),
        'loot_zone': dict(cfg=_c5(inventory={'slots': 4}, safe_zone=LOOT_ZONE), driver=drive_loot_zone),
    }[name]
    return SimpleNamespace(name=name, **s)


SCENARIOS = ('handover_2v2', 'handover_ffa4', 'builder', 'builder_2v2', 'loot', 'loot_zone')

# Coverage floors: half of what the oracle reaches on the CPU test's seeds
# (8 seeds x 300 steps), and at least one; both numbers are in
# profiles/items_laws.txt.
FLOORS = {
    # the oracle: give_taken 440, give_lost 4, give_refused 58, give_two_hands 114
    'handover_2v2': {'give_taken': 220, 'give_lost': 2, 'give_refused': 29, 'give_two_hands': 57},
    # the oracle: give_to_agent 18, give_to_heal 18, give_to_box 37, give_to_box_item 3, give_to_placed 3,
    # give_to_non_agent 61, double_pickups 1
    'handover_ffa4': {'give_to_agent': 9, 'give_to_heal': 9, 'give_to_box': 18, 'give_to_box_item': 1, 'give_to_placed': 1,
        'give_to_non_agent': 30, 'double_pickups': 1},
    # the oracle: placements 32, place_q0 10, place_q1 5, place_q2 9, place_q3 8, placed_hit 5, owner_breaks 11,
    # stranger_swings 7, replaced 7
    'builder': {'placements': 16, 'place_q0': 5, 'place_q1': 2, 'place_q2': 4, 'place_q3': 4, 'placed_hit': 2, 'owner_breaks': 5,
        'stranger_swings': 3, 'replaced': 3},
    # the oracle: placements 34, place_q0 12, place_q1 8, place_q2 6, place_q3 8, placed_hit 4, owner_breaks 30,
    # mate_breaks 7, stranger_swings 68, replaced 10
    'builder_2v2': {'placements': 17, 'place_q0': 6, 'place_q1': 4, 'place_q2': 3, 'place_q3': 4, 'placed_hit': 2,
        'owner_breaks': 15, 'mate_breaks': 3, 'stranger_swings': 34, 'replaced': 5},
    # the oracle: deaths_depth1 5, deaths_depth2 7, deaths_depth3p 4, drop_box_items 4, drop_found 3, drops_contact 19
    'loot': {'deaths_depth1': 2, 'deaths_depth2': 3, 'deaths_depth3p': 2, 'drop_box_items': 2, 'drop_found': 1, 'drops_contact': 9},
    # the oracle: deaths_depth1 35, deaths_depth2 6, drops_free 36
    'loot_zone': {'deaths_depth1': 17, 'deaths_depth2': 3, 'drops_free': 18},
    # the oracle: deaths_depth1 28, deaths_depth2 7, drops_free 37
    'loot_ffal': {'deaths_depth1': 14, 'deaths_depth2': 3, 'drops_free': 18},
}


def run(sc, reset, step, seeds, n_steps, record=None):
    """Drive N envs for n_steps with the scenario's controller and apply the
    laws to every step.  reset() -> obs [N, A, D]; step(actions) -> (obs,
    rewards, done [N]) with done envs already reset.  record(t, actions, obs,
    rewards, done), if given, sees every step."""
    C = ir.constants(sc.cfg)
    st = Stats()
    rng = np.random.default_rng(1913 + len(sc.name))
    seeds = np.asarray(list(seeds))
    prev = ir.decode(reset(), C)
    L = Ledger(prev.N, C)
    every = np.ones(prev.N, dtype=bool)
    law_reset(C, prev, every, st)
    L.reset(every, prev)
    law_tops(C, prev, L, every, st, -1)
    scratch = Stats()
    for t in range(n_steps):
        a = sc.driver(t, prev, seeds, rng, C)
        obs, rew, done = step(a)
        if record is not None:
            record(t, a, obs, rew, done)
        done = np.asarray(done, dtype=bool)
        new = ir.decode(obs, C)
        led = rl.law_ledger(C, prev, new, a, ~done, L.rules, scratch, t)   # for its swings and cooldowns; judged elsewhere
        law_items(C, prev, new, a, ~done, led, L, st, t)
        law_reset(C, new, done, st)
        L.reset(done, new)
        law_tops(C, new, L, every, st, t)
        st.add('env_steps', (~done).sum())
        st.add('episodes', done.sum())
        st.worst['max_depth'] = max(st.worst.get('max_depth', 0), max(len(s) for e in L.stack for s in e))
        st.worst['max_box_items'] = max(st.worst.get('max_box_items', 0), int(new.bitems_on.sum(-1).max()) if C.B else 0)
        st.worst['max_heals'] = max(st.worst.get('max_heals', 0), int(new.heals_on.sum(-1).max()) if C.H else 0)
        prev = new
    st.refused_envs = sorted(L.refused_envs)
    return st


VIOLATIONS = ('reset_wrong', 'place_wrong', 'top_wrong', 'conserve_wrong', 'drop_wrong', 'owner_wrong', 'box_vanished')


def check(sc, st):
    """The assertions both suites make on a finished run."""
    rep = st.report()
    c = st.count
    for k in VIOLATIONS:
        assert c.get(k, 0) == 0, (sc.name, k, st.where.get(k), rep)
    C = ir.constants(sc.cfg)
    if C.ownership and C.randomized:     # law K needs an env's shapes to differ; they are random draws here
        assert c['reset_shapes_clash'] == 0, (sc.name, rep)
    for k in ('place_pos', 'drop_radius'):
        if k in st.worst:
            assert st.worst[k] <= TOL[k], (sc.name, k, st.worst[k], st.where.get(k), rep)
    assert c.get('give_graze', 0) <= LIDAR_GRAZE_SHARE * (c.get('give_events', 0) + c.get('placements', 0)), (sc.name, rep)
    assert c.get('unknown_steps', 0) <= UNKNOWN_SHARE * c['agent_steps'], (sc.name, rep)
    assert c.get('conserve_skipped', 0) <= UNJUDGED_SHARE * c['env_steps'], (sc.name, rep)
    for k, floor in FLOORS[sc.name].items():
        assert c.get(k, 0) >= floor > 0, (sc.name, k, c.get(k, 0), floor, rep)
