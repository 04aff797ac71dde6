"""TEST INFRASTRUCTURE ONLY: the physical laws an env step must obey, the
scenarios that drive envs into contact, and the loop that applies the one to
the other.  Shared by tests/test_physics_reference.py (the C oracle, CPU) and
tests/test_gpu_physics_laws.py (the HIP kernels).

Every law works on two consecutive decoded observation rows (physics_ref.decode)
and the actions between them, knows nothing of the code that produced them, and
returns deviations in fp32 ulps of the quantity's magnitude,
np.spacing(np.float32(max(|q|, 1))).  Laws skip env-steps whose `done` is set
(the new row is then a fresh episode) and agents not alive in both rows."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import physics_ref as pr
from masurvival.config import C3_CONFIG, C5_CONFIG

# Box2D's constants, for the one bound that is derived from them
LINEAR_SLOP = 0.005
POLYGON_RADIUS = 2.0 * LINEAR_SLOP
TOI_TOLERANCE = 0.25 * LINEAR_SLOP
FAT = 0.1            # b2_aabbExtension: what the broad phase calls "near"
NEAR_BOX = 0.02      # coverage: an agent this close to a box's skin is at the box
CORNER = 0.52        # coverage: an agent this close to two walls is in a corner
SLEEP_LIN, SLEEP_ANG = 0.01, math.radians(2.0)

# Tolerances in fp32 ulps: 4 x the worst deviation of the unmodified oracle over
# the CPU test's scenarios; measured values, coverage counts and the mutants
# each law catches are in profiles/physics_laws.txt.  Whatever is measured,
# free flight, momentum and pairs stay <= 16 ulp and lidar <= 1e-4 relative depth.
TOL = {
    'ff_vel': 7.4, 'ff_spin': 9.2, 'ff_pos': 5.7, 'ff_ang': 4.5,   # oracle worst 1.848, 2.288, 1.415, 1.112
    'momentum': 12.9,                                               # 3.206
    'pair_speed': 0.0, 'pair_sink': 8.1,                            # 0 (never approaching), 2.024
    'lidar': 5.3e-5,                                                # 1.317e-5 relative depth
}
# no new penetration of statics: epsilon covers only the rounding of the fp32
# rows, a few ulp of the coordinate; 0.49375 itself is Box2D's TOI target
# r + polygonRadius - 3 slop - tolerance and is not tuned
STATIC_EPS_ULP = 4.0
LIDAR_GRAZE = 1e-4
LIDAR_GRAZE_SHARE = 0.005


def toi_gap(C):
    return C.r + POLYGON_RADIUS - 3.0 * LINEAR_SLOP - TOI_TOLERANCE


def ulps(err, mag):
    return np.abs(err) / np.spacing(np.maximum(np.abs(mag), 1.0).astype(np.float32)).astype(np.float64)


def _norm(v):
    return np.sqrt((v * v).sum(-1))


class Stats:
    """Worst deviation per law quantity (with where it happened) and counts."""

    def __init__(self):
        self.worst, self.where, self.count = {}, {}, {}

    def dev(self, key, values, mask, t):
        self.worst.setdefault(key, 0.0)
        if mask.any():
            v = np.where(mask, values, -1.0)
            assert not np.isnan(v).any(), (key, t)
            k = int(v.argmax())
            if v.flat[k] > self.worst[key]:
                self.worst[key] = float(v.flat[k])
                self.where[key] = (t,) + tuple(int(x) for x in np.unravel_index(k, v.shape))

    def add(self, key, n):
        self.count[key] = self.count.get(key, 0) + int(n)

    def report(self):
        w = ', '.join(f'{k}={v:.4g}@{self.where.get(k)}' for k, v in sorted(self.worst.items()))
        c = ', '.join(f'{k}={v}' for k, v in sorted(self.count.items()))
        return f'worst [{w}] counts [{c}]'


def make_step(prev, new, actions, done, C, t):
    """Everything the laws share about one env step of N envs."""
    S = SimpleNamespace(prev=prev, new=new, actions=actions, C=C, t=t, valid=~np.asarray(done, dtype=bool))
    S.both = prev.alive & new.alive & S.valid[:, None]
    S.wg = (pr.wall_gaps(prev, C), pr.wall_gaps(new, C))
    S.bg = (pr.box_gaps(prev), pr.box_gaps(new))
    S.pd = (pr.pair_dist(prev), pr.pair_dist(new))
    # near a static: a wall, or a box of either row at either end of the step.  A box placed in this step
    # is in the new row alone and shoves the agent it lands on out of itself, perhaps beyond the margin; a
    # box broken in this step is in the previous row alone and was still solid while the agent moved.
    S.box_changed = (prev.box_raw != new.box_raw).any(-1)
    cross = (pr.box_gaps(prev, new), pr.box_gaps(new, prev))
    inf = np.full(prev.pos.shape[:2] + (1,), np.inf)
    gaps = np.concatenate(S.wg + S.bg + cross + (inf,), -1)
    S.near_static = gaps.min(-1) < C.r + FAT
    S.near_changed_box = S.box_changed[:, None] & (np.concatenate(S.bg + cross + (inf,), -1).min(-1) < C.r + FAT)
    S.near_pair = (S.pd[0].min(-1) < 2 * C.r + FAT) | (S.pd[1].min(-1) < 2 * C.r + FAT)
    S.ff = pr.free_flight(prev, actions, C)
    return S


def _free_flight_dev(S):
    v, w, pos, ang = S.ff
    new = S.new
    dv = ulps(np.abs(new.vel - v).max(-1), _norm(v))
    dw = ulps(new.omega - w, w)
    # sleep: a body that stayed below both thresholds for half a second has its velocities zeroed
    asleep = (_norm(v) <= SLEEP_LIN) & (np.abs(w) <= SLEEP_ANG) & (new.vel == 0).all(-1) & (new.omega == 0)
    dv, dw = np.where(asleep, 0.0, dv), np.where(asleep, 0.0, dw)
    dp = ulps(np.abs(new.pos - pos).max(-1), np.abs(pos).max(-1))
    da = ulps(new.angle - ang, ang)
    return {'vel': dv, 'spin': dw, 'pos': dp, 'ang': da}


def law_free_flight(S, st):
    """Law 1: an agent-step with nothing within the broad-phase margin, in the
    previous or the new row, follows the closed form."""
    judged = S.both & ~S.near_static & ~S.near_pair
    for k, d in _free_flight_dev(S).items():
        st.dev('ff_' + k, d, judged, S.t)
    st.add('alive_steps', S.both.sum())
    st.add('ff_judged', judged.sum())
    st.add('ff_excluded', (S.both & ~judged).sum())


def law_fast_path(S, st, gen_flags):
    """Law 2: an env the kernels stepped on their contact-free fast path
    follows the closed form for all its alive agents, with no filter."""
    fast = np.asarray(gen_flags) == 0
    judged = S.both & fast[:, None]
    for k, d in _free_flight_dev(S).items():
        st.dev('fast_' + k, d, judged, S.t)
    st.add('fast_env_steps', (fast & S.valid).sum())
    st.add('general_env_steps', (~fast & S.valid).sum())


def law_momentum(S, st):
    """Law 3: with no alive agent near a wall or a box, the agents' summed
    momentum changes by damping and motor impulses alone, contacts between
    agents included."""
    same = ((S.prev.alive == S.new.alive) & (S.prev.present == S.prev.alive) &
            (S.new.present == S.new.alive)).all(-1) & S.prev.alive.any(-1)  # no body comes, goes or lingers dead
    env = S.valid & same & ~(S.near_static & (S.prev.alive | S.new.alive)).any(-1)
    d = pr.momentum_defect(S.prev, S.actions, S.new, S.C)
    mag = (S.C.m * _norm(S.new.vel) * S.new.alive).sum(-1)
    st.dev('momentum', ulps(np.abs(d).max(-1), mag), env, S.t)
    st.add('momentum_env_steps', env.sum())
    touching = env & (np.minimum(S.pd[0], S.pd[1]).min(axis=(1, 2)) <= 2 * S.C.r)
    st.add('momentum_contact_env_steps', touching.sum())


def law_statics(S, st):
    """Law 4: no agent goes deeper into a wall, or into a box that is there in
    both rows, than the TOI target or than it already was.

    Boxes: only on steps whose `boxes` and `boxes_mask` blocks are identical
    in both rows (slots shift when a box breaks or is placed).  Walls: always,
    but for an agent next to a box on the step that placed or broke one: a box
    placed onto an agent overlaps it from the start, no sweep is involved, and
    the position solver pushes the agent out of the box by up to its radius,
    into a wall if one is behind it.  That is Box2D's answer to spawning a
    body into another, not a missed time of impact."""
    C = S.C
    coord = np.abs(S.new.pos).max(-1)[..., None]
    lack = np.minimum(S.wg[0], toi_gap(C)) - S.wg[1]
    judged = np.broadcast_to((S.both & ~S.near_changed_box)[..., None], lack.shape)
    st.dev('wall_sink', ulps(np.maximum(lack, 0.0), coord), judged, S.t)
    if S.bg[0].shape[-1]:
        same = ~S.box_changed
        lack = np.minimum(S.bg[0], toi_gap(C)) - S.bg[1]
        ok = S.both[..., None] & same[:, None, None] & np.isfinite(S.bg[0]) & np.isfinite(S.bg[1])
        st.dev('box_sink', ulps(np.maximum(np.where(ok, lack, 0.0), 0.0), coord), ok, S.t)
    g = np.where((S.both & ~S.near_changed_box)[..., None], S.wg[1], np.inf)
    st.worst['min_wall_gap'] = min(st.worst.get('min_wall_gap', np.inf), float(g.min()) if g.size else np.inf)
    st.add('corner_steps', (S.both & ((S.wg[1] < CORNER).sum(-1) >= 2)).sum())
    if S.bg[1].shape[-1]:
        st.add('box_near_steps', (S.both & (S.bg[1].min(-1) < C.r + NEAR_BOX)).sum())


def law_pairs(S, st):
    """Law 5: a pair that touches in both rows, away from statics and from
    every third agent, neither approaches along its centre line nor sinks
    further.

    Touching in the new row alone is the first discrete contact step, where
    overlap is legitimate.  A third body within the broad-phase margin of
    either member makes the island a chain of contacts, which ten sequential
    impulse iterations do not solve exactly: an agent squeezed between two
    others sinks by millimetres per step.  That is Box2D's solver, not an
    error, so the law judges two-body islands only, whose single contact every
    iteration solves exactly."""
    C = S.C
    A = S.prev.pos.shape[1]
    upper = np.triu(np.ones((A, A), dtype=bool), 1)[None]
    free = S.both & ~S.near_static
    alone = (np.minimum(S.pd[0], S.pd[1]) < 2 * C.r + FAT).sum(-1) == 1
    free = free & alone
    judged = upper & free[:, :, None] & free[:, None, :] & (S.pd[0] <= 2 * C.r) & (S.pd[1] <= 2 * C.r)
    vn = pr.pair_normal_speed(S.new)
    rel = _norm(S.new.vel[:, None] - S.new.vel[:, :, None])
    st.dev('pair_speed', ulps(np.maximum(-vn, 0.0), rel), judged, S.t)
    with np.errstate(invalid='ignore'):
        sink = np.where(judged, S.pd[0] - S.pd[1], 0.0)
    st.dev('pair_sink', ulps(np.maximum(sink, 0.0), 1.0), judged, S.t)
    st.add('pair_steps', judged.sum())


def law_lidar(rows, C, st, t):
    """Law 6: every lidar column is the fp64 closest hit, with the same
    hit/miss decision.  A ray within LIDAR_GRAZE of grazing something may
    disagree; such rays are counted."""
    f, graze = pr.lidar_ref(rows, C, LIDAR_GRAZE)
    o = rows.lidars
    alive = np.broadcast_to(rows.present[..., None], f.shape)
    agree = (f < 1.0) == (o < 1.0)
    err = np.abs(f - o)
    st.dev('lidar', err, alive & agree & ~graze, t)
    bad = alive & (~agree | (err > TOL['lidar']))
    st.add('lidar_rays', alive.sum())
    st.add('lidar_hits', (alive & (o < 1.0)).sum())
    st.add('lidar_wrong', (bad & ~graze).sum())
    st.add('lidar_excused', (bad & graze).sum())


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------
MELEE = {'range': 2, 'damage': 20, 'cooldown': 40, 'drift': True}
BARE = {
    'heals': {'reset_spawns': {'n_items': 0, 'item_size': 0.5}, 'heal': {'healing': 50}},
    'boxes': {'reset_spawns': {'n_boxes': 0, 'box_size': 1}, 'ownership': False,
              'item': {'item_size': 0.5, 'offset': 0.75}, 'health': 20},
    'melee': MELEE}
HI = np.array([3, 3, 3, 2, 2, 2])


def _lid_ffa4():
    from test_gpu_lidars_batch import LID_FFA4
    return {k: v for k, v in LID_FFA4.items() if k != 'safe_zone'}  # the default safe zone


def drive_bare_duel(t, rows, seeds, rng, C):
    if (t // 150) % 2 == 0:
        return pr.duel(rows)
    c = 0.4 * C.floor
    corners = np.array([[-c, -c], [c, c]])
    return pr.seek(rows, np.broadcast_to(corners[None], rows.pos.shape))


def drive_bare_walls(t, rows, seeds, rng, C):
    """agent 0: a point 2 m behind a wall, agent 1: 2 m outside a corner; the
    side turns with the env's seed and the targets are mirrored every 120 steps"""
    out = C.floor / 2.0 + 2.0
    s = np.asarray(seeds)
    along = ((s * 37) % 13 - 6.0) / 6.0 * 0.3 * C.floor
    tg = np.stack([np.stack([np.full(len(s), out), along], -1), np.full((len(s), 2), out)], axis=1)
    tg = pr._rot((s % 4)[:, None] * (math.pi / 2.0), tg)
    if (t // 120) % 2:
        tg = -tg
    return pr.seek(rows, tg)


def drive_duel(t, rows, seeds, rng, C):
    return pr.duel(rows)


def drive_boxes(t, rows, seeds, rng, C):
    if (t // 60) % 2 == 0:
        return pr.seek(rows, pr.nearest(rows, rows.box_pos, rows.box_on))
    return rng.integers(0, HI, size=rows.pos.shape[:2] + (6,)).astype(np.int8)


def drive_random(t, rows, seeds, rng, C):
    return rng.integers(0, HI, size=rows.pos.shape[:2] + (6,)).astype(np.int8)


def scenario(name):
    s = {
        'bare_duel': dict(cfg=dict(BARE), driver=drive_bare_duel, lidar_only=False),
        'bare_walls': dict(cfg=dict(BARE), driver=drive_bare_walls, lidar_only=False),
        '2v2_duel': dict(cfg=C3_CONFIG, driver=drive_duel, lidar_only=False),
        'ffa4_boxes': dict(cfg=C5_CONFIG, driver=drive_boxes, lidar_only=False),
        'ffa4_lidar': dict(cfg=None, driver=drive_random, lidar_only=True),
    }[name]
    if s['cfg'] is None:
        s['cfg'] = _lid_ffa4()
    return SimpleNamespace(name=name, **s)


SCENARIOS = ('bare_duel', 'bare_walls', '2v2_duel', 'ffa4_boxes', 'ffa4_lidar')

# Coverage floors: half of what the oracle reaches on the CPU test's seeds
# (8 seeds x 300 steps; ffa4_lidar 6 x 80); both numbers are in
# profiles/physics_laws.txt.  ff_share: the least share of alive agent-steps
# law 1 must judge: 30 % in the duels, 80 % in ffa4_lidar; below that the
# contact filter would be too wide to mean anything.
FLOORS = {
    'bare_duel': {'pair_steps': 98, 'ff_share': 0.30},        # the oracle: 197
    'bare_walls': {'corner_steps': 258},                      # 517
    '2v2_duel': {'pair_steps': 482, 'ff_share': 0.30},        # 964
    'ffa4_boxes': {'box_near_steps': 1523},                   # 3047
    'ffa4_lidar': {'ff_share': 0.80, 'lidar_hits': 7585},     # 15170
}


def run(sc, reset, step, seeds, n_steps, gen_flags=None, record=None):
    """Drive N envs for n_steps with the scenario's controller and apply the
    laws to every step.  reset() -> obs [N, A, D]; step(actions) -> (obs,
    rewards, done [N]) with done envs already reset; gen_flags() -> [N] after
    a step (GPU only).  record(t, actions, obs, rewards, done), if given,
    sees every step.  Returns the Stats."""
    C = pr.constants(sc.cfg)
    st = Stats()
    rng = np.random.default_rng(20240 + len(sc.name))
    seeds = np.asarray(list(seeds))
    prev = pr.decode(reset(), C)
    if C.lidars:
        law_lidar(prev, C, st, -1)
    for t in range(n_steps):
        a = sc.driver(t, prev, seeds, rng, C)
        obs, rew, done = step(a)
        if record is not None:
            record(t, a, obs, rew, done)
        new = pr.decode(obs, C)
        S = make_step(prev, new, a, done, C, t)
        law_free_flight(S, st)
        if gen_flags is not None:
            law_fast_path(S, st, gen_flags())
        if C.lidars:
            law_lidar(new, C, st, t)
        if not sc.lidar_only:
            law_momentum(S, st)
            law_statics(S, st)
            law_pairs(S, st)
        st.add('env_steps', S.valid.sum())
        prev = new
    return st


def check(sc, st):
    """The assertions both suites make on a finished run."""
    rep = st.report()
    for k in ('ff_vel', 'ff_spin', 'ff_pos', 'ff_ang', 'momentum', 'pair_speed', 'pair_sink', 'lidar'):
        if k in st.worst:
            assert st.worst[k] <= TOL[k], (sc.name, k, st.worst[k], st.where.get(k), rep)
    for k in ('fast_vel', 'fast_spin', 'fast_pos', 'fast_ang'):
        if k in st.worst:
            assert st.worst[k] <= TOL['ff_' + k[5:]], (sc.name, k, st.worst[k], st.where.get(k), rep)
    for k in ('wall_sink', 'box_sink'):
        if k in st.worst:
            assert st.worst[k] <= STATIC_EPS_ULP, (sc.name, k, st.worst[k], st.where.get(k), rep)
    c = st.count
    if 'lidar_rays' in c:
        assert c['lidar_wrong'] == 0, (sc.name, rep)
        assert c['lidar_excused'] <= LIDAR_GRAZE_SHARE * c['lidar_rays'], (sc.name, rep)
    # coverage: the run reached the regime it is named for
    assert c['ff_judged'] > 0 and c['ff_excluded'] > 0, (sc.name, rep)
    for k, floor in FLOORS[sc.name].items():
        if k == 'ff_share':
            assert c['ff_judged'] >= floor * c['alive_steps'], (sc.name, k, rep)
        else:
            assert c[k] >= floor > 0, (sc.name, k, c[k], floor, rep)
