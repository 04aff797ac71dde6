"""Synthetic observation rows for the scripted bots' tests: random rows that
cover the rule's branches, and hand-made edge rows (exact ties, a target at the
agent's own position, thresholds met exactly).  Every value is rounded to bf16,
so the fp64 reference (tests/bot_ref.py) and the kernel read the same numbers."""
import math

import numpy as np

from bot_play import bf16_round
from masurvival.layout import obs_layout

SENTINEL = 768.0  # what the columns at and past obs_dim hold (bf16-exact)


def stride_of(obs_dim, wider=False):
    """The policies' row stride (room for a bias column, rounded up to 16), or a wider one."""
    dx = 16 * ((obs_dim + 1 + 15) // 16)
    return dx + 24 if wider else dx


def layout_of(cs):
    return obs_layout(int(cs.n_agents), int(cs.n_heals), int(cs.n_boxes), bool(cs.teams), int(cs.lidar_n_lasers))


def random_rows(cs, n_envs, seed, stride=None):
    """fp32 [n_envs * n_agents, stride] of bf16-exact values: columns [0, obs_dim)
    an observation-like row per agent, the rest SENTINEL."""
    rng = np.random.default_rng(seed)
    A, H, teams = int(cs.n_agents), int(cs.n_heals), int(bool(cs.teams))
    D, lay = layout_of(cs)
    stride = stride or stride_of(D)
    rec, o = 8 + teams, 1 + teams
    half = float(cs.floor_size) / 2.0 - 0.5
    x = rng.normal(0.0, 3.0, size=(n_envs, A, stride))  # sections the rule never reads hold noise
    x[:, :, D:] = SENTINEL
    # the agents of an env: pose uniform in the room; a dead agent shows zeros
    health = rng.integers(1, int(cs.agent_health) + 1, size=(n_envs, A)).astype(np.float64)
    health[rng.random((n_envs, A)) < 0.15] = 0.0
    low = rng.random((n_envs, A)) < 0.3
    health[low & (health > 0)] = rng.integers(1, 60, size=int((low & (health > 0)).sum()))
    body = np.zeros((n_envs, A, rec))
    body[:, :, 0] = np.arange(A)
    if teams:
        body[:, :, 1] = (np.arange(A) >= A // 2).astype(np.float64)
    body[:, :, o] = health
    body[:, :, o + 1:o + 3] = rng.uniform(-half, half, size=(n_envs, A, 2))
    crowd = rng.random(n_envs) < 0.3  # some envs fight at close range
    body[crowd, :, o + 1:o + 3] = rng.uniform(-2.0, 2.0, size=(int(crowd.sum()), A, 2)) + rng.uniform(
        -5, 5, size=(int(crowd.sum()), 1, 2))
    body[:, :, o + 3] = rng.uniform(-math.pi, math.pi, size=(n_envs, A))
    body[:, :, o + 4:o + 6] = rng.normal(0.0, 1.0, size=(n_envs, A, 2))
    body[:, :, o + 6] = rng.normal(0.0, 2.0, size=(n_envs, A))
    body[health <= 0, o:] = 0.0
    zone = np.zeros((n_envs, 6))
    zone[:, 0:2] = rng.uniform(-5.0, 5.0, size=(n_envs, 2))
    zone[:, 2] = rng.choice([0.0, 1.0, 2.5, 5.0, 10.0, 10.0], size=n_envs)
    zone[:, 3:5] = rng.uniform(-5.0, 5.0, size=(n_envs, 2))
    zone[:, 5] = rng.choice([0.0, 1.0, 2.5, 5.0], size=n_envs)
    if H > 0:
        heals = rng.uniform(-half, half, size=(n_envs, H, 2))
        heals[crowd] = heals[crowd] * 0.3
    for i in range(A):
        x[:, i, lay['agent'][0]:lay['agent'][0] + rec] = body[:, i]
        others = [j for j in range(A) if j != i]
        x[:, i, lay['others'][0]:lay['others'][0] + (A - 1) * rec] = body[:, others].reshape(n_envs, -1)
        x[:, i, lay['others_mask'][0]:lay['others_mask'][0] + A - 1] = (rng.random((n_envs, A - 1)) < 0.3)
        x[:, i, lay['zone'][0]:lay['zone'][0] + 6] = zone
        if H > 0:
            mask = (rng.random((n_envs, H)) < 0.4).astype(np.float64)
            mask[rng.random(n_envs) < 0.2] = 1.0  # no heal visible
            shown = np.where(mask[:, :, None] == 0, heals, 0.0) if not cs.omniscient else heals
            x[:, i, lay['heals'][0]:lay['heals'][0] + 2 * H] = shown.reshape(n_envs, -1)
            x[:, i, lay['heals_mask'][0]:lay['heals_mask'][0] + H] = mask
            has = rng.random(n_envs) < 0.5
            x[:, i, lay['heal_slot'][0]] = np.where(has, float(cs.healing), 0.0)
            x[:, i, lay['heal_slot_mask'][0]] = np.where(has, 0.0, 1.0)
    return bf16_round(x.reshape(n_envs * A, stride))


def edge_rows(cs, stride=None):
    """Hand-made rows of the 2v2 teams config (others of agent 0: [1, 2, 3],
    enemies 2 and 3 at others' indices 1 and 2), every number a small multiple
    of 1/4 and the heading 0 (cos 1, sin 0 exactly), so that fp32 and fp64 agree
    to the bit on every tie.  Returns (rows [n * 4, stride], labels); only
    agent 0's row of each env is the case, the other rows are dead selves."""
    A, H = int(cs.n_agents), int(cs.n_heals)
    assert A == 4 and cs.teams and H == 4
    D, lay = layout_of(cs)
    stride = stride or stride_of(D)
    rec, o = 9, 2

    def env(pos=(1.0, 2.0), hp=100, theta=0.0, w=0.0, zone=(0.0, 0.0, 10.0), others=(), heals=(), slot=False):
        r = np.zeros((A, stride))
        r[:, D:] = SENTINEL
        r[:, lay['others_mask'][0]:lay['others_mask'][0] + 3] = 1.0
        r[:, lay['heals_mask'][0]:lay['heals_mask'][0] + 4] = 1.0
        r[:, lay['heal_slot_mask'][0]] = 1.0
        a = lay['agent'][0]
        r[0, a:a + rec] = [0, 0, hp, pos[0], pos[1], theta, 0, 0, w]
        r[0, lay['zone'][0]:lay['zone'][0] + 3] = zone
        for j in range(3):  # others of agent 0: agents 1 (own team), 2, 3
            r[0, lay['others'][0] + j * rec:lay['others'][0] + j * rec + 2] = [j + 1, int(j + 1 >= 2)]
        for j, ohp, ox, oy in others:
            r[0, lay['others'][0] + j * rec + o:lay['others'][0] + j * rec + o + 3] = [ohp, ox, oy]
            r[0, lay['others_mask'][0] + j] = 0.0
        for k, hx, hy in heals:
            r[0, lay['heals'][0] + 2 * k:lay['heals'][0] + 2 * k + 2] = [hx, hy]
            r[0, lay['heals_mask'][0] + k] = 0.0
        if slot:
            r[0, lay['heal_slot'][0]], r[0, lay['heal_slot_mask'][0]] = float(cs.healing), 0.0
        return r

    cases = [
        ('enemy exactly at the own position', env(others=[(1, 50, 1.0, 2.0)])),
        ('heal exactly at the own position', env(heals=[(0, 1.0, 2.0)])),
        ('mirrored enemies: the lower index', env(others=[(1, 50, 4.0, 3.0), (2, 50, -2.0, 1.0)])),
        ('mirrored enemies, order swapped', env(others=[(1, 50, -2.0, 1.0), (2, 50, 4.0, 3.0)])),
        ('enemies with dx and dy swapped', env(others=[(1, 50, 2.0, 5.0), (2, 50, 4.0, 3.0)])),
        ('own team nearer than the enemy', env(others=[(0, 50, 1.5, 2.0), (2, 50, 4.0, 3.0)])),
        ('dead enemy nearer than the living', env(others=[(1, 0, 1.5, 2.0), (2, 50, -4.0, 2.0)])),
        ('mirrored heals', env(heals=[(1, 4.0, 3.0), (3, -2.0, 1.0)])),
        ('mirrored heals, order swapped', env(heals=[(0, -2.0, 1.0), (2, 4.0, 3.0)])),
        ('heal and enemy: the forager takes the heal', env(others=[(1, 50, 2.0, 2.0)], heals=[(2, 1.0, 5.0)])),
        ('enemy at exactly 4 m', env(others=[(2, 50, 5.0, 2.0)])),
        ('enemy at 4.25 m', env(others=[(2, 50, 5.25, 2.0)])),
        ('enemy at exactly the standoff', env(others=[(1, 50, 2.25, 2.0)])),
        ('enemy at exactly the reach', env(others=[(1, 50, 3.5, 2.0)])),
        ('enemy just past the reach', env(others=[(1, 50, 3.75, 2.0)])),
        ('enemy behind', env(others=[(1, 50, -3.0, 2.0)])),
        ('zone radius 0, at the centre', env(pos=(1.0, 2.0), zone=(1.0, 2.0, 0.0), others=[(1, 50, 3.0, 2.0)])),
        ('zone radius 0, off the centre', env(zone=(3.0, 2.0, 0.0), others=[(1, 50, 1.0, 4.0)])),
        ('exactly on the margin', env(pos=(4.0, 0.0), zone=(0.0, 0.0, 5.0), others=[(1, 50, 6.0, 0.0)])),
        ('a quarter past the margin', env(pos=(4.25, 0.0), zone=(0.0, 0.0, 5.0), others=[(1, 50, 6.0, 0.0)])),
        ('zone radius below the margin', env(zone=(1.0, 2.0, 0.5), heals=[(0, 1.0, 3.0)])),
        ('heal outside the margin', env(zone=(0.0, 0.0, 5.0), heals=[(0, 4.5, 0.0), (1, -3.0, 2.0)])),
        ('arrived at the zone centre', env(pos=(0.25, 0.0), zone=(0.0, 0.0, 0.0))),
        ('dead self', env(hp=0, others=[(1, 50, 2.0, 2.0)], heals=[(0, 1.0, 3.0)], slot=True)),
        ('use at exactly the threshold', env(hp=50, slot=True)),
        ('no use one above the threshold', env(hp=51, slot=True)),
        ('no use without a heal in the slot', env(hp=10)),
        ('nothing in sight', env()),
        ('turning fast: the damping flips the turn', env(w=4.0, others=[(1, 50, 4.0, 3.0)])),
    ]
    rows = np.concatenate([r for _, r in cases])
    return bf16_round(rows), [name for name, _ in cases]
