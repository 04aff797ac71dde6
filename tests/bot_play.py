"""Scripted bots on the CPU oracle: tests/bot_ref.py drives OracleEnv on
bf16-rounded rows, every seed's env stepped in lockstep, and every row the
bots act on is also given to masurvival.bots.bot_actions_reference.
`PYTHONPATH=gym-ma-survival-2d_amd:oracle python tests/bot_play.py` prints the
table of profiles/bots.txt."""
import numpy as np

import bot_ref
from masurvival.config import C1_CONFIG, C3_CONFIG, ResolvedConfig, pcg64_state

SEEDS = 32
NONOMNI_2V2 = dict(C3_CONFIG, observation={'omniscent': False})
CONFIGS = {'1v1': C1_CONFIG, '2v2': C3_CONFIG, '2v2_nonomniscient': NONOMNI_2V2}
PAIRINGS = (('hunter', 'idle'), ('forager', 'idle'), ('hunter', 'forager'), ('idle', 'idle'))


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def play(config, kinds, seeds=SEEDS, max_steps=6000, check_reference=True):
    """Side 0 (agents [0, A/2)) plays kinds[0], side 1 kinds[1], one episode per
    seed.  Wins by Match's rule: the side whose agents' summed return is larger."""
    import torch
    from masurvival.bots import bot_actions_reference
    from oracle import OracleEnv, counters
    rc = ResolvedConfig(config)
    cs, A = rc.to_struct(), rc.n_agents
    envs = [OracleEnv(cs, pcg64_state(s)) for s in range(seeds)]
    obs = np.stack([e.reset() for e in envs])
    running = np.ones(seeds, dtype=bool)
    ret, length = np.zeros((seeds, A)), np.zeros(seeds, dtype=np.int64)
    side = np.array([int(a >= A // 2) for a in range(A)])
    rows = near = mismatch = 0
    counters(True)
    for _ in range(max_steps):
        x = bf16_round(obs).reshape(seeds * A, -1)
        acts = np.zeros((seeds * A, 6), dtype=np.int8)
        for s in (0, 1):
            kind = bot_ref.KINDS[kinds[s]]
            a, nr = bot_ref.bot_ref(kind, x, cs)
            sel = np.tile(side == s, seeds)
            acts[sel] = a[sel]
            counted = sel & np.repeat(running, A)
            rows += int(counted.sum())
            near += int(nr[counted].sum())
            if check_reference:
                b = bot_actions_reference(kind, torch.from_numpy(x), rc).numpy()
                mismatch += int(((a != b).any(axis=1) & counted & ~nr).sum())
        acts = acts.reshape(seeds, A, 6)
        for i, e in enumerate(envs):
            if running[i]:
                o, r, d = e.step(acts[i])
                obs[i], ret[i], length[i] = o, ret[i] + r, length[i] + 1
                running[i] = not d
        if not running.any():
            break
    s0, s1 = ret[:, side == 0].sum(1), ret[:, side == 1].sum(1)
    return {'episodes': seeds, 'finished': int((~running).sum()), 'wins': [int((s0 > s1).sum()), int((s1 > s0).sum())],
            'draws': int((s0 == s1).sum()), 'mean_length': float(length.mean()),
            'heal_used': int(counters()['heal_used']), 'rows': rows, 'near': near, 'mismatch': mismatch}


def play_all(check_reference=True):
    return {(name, pair): play(cfg, pair, check_reference=check_reference)
            for name, cfg in CONFIGS.items() for pair in PAIRINGS}


if __name__ == '__main__':
    for (name, pair), r in play_all().items():
        print(f'{name:18s} {pair[0]:8s} vs {pair[1]:8s} wins {r["wins"][0]:2d}:{r["wins"][1]:2d} draws {r["draws"]:2d} '
              f'of {r["episodes"]} (finished {r["finished"]})  mean length {r["mean_length"]:7.1f}  heals used '
              f'{r["heal_used"]:3d}  near rows {r["near"]}/{r["rows"]} = {100.0 * r["near"] / r["rows"]:.4f} %  '
              f'reference mismatches {r["mismatch"]}')
