"""How many TOI events of a SolveTOI call repeat the event before them bit for
bit (the evidence behind the repeated-event skip in toi_agent_group,
csrc/mas_physics.h).

Builds an INSTRUMENTED COPY of the C oracle in a temp dir.  After each TOI
event of world_toi_agent the copy compares ten values -- the sweep (c0, a0,
c, a, alpha0) and the agent's v and w -- and the min static with those the
previous event of the same call left.  It replays (a) the PPO-regime env
whose SolveTOI reaches the sub-step cap (tests/golden/wedged_2v2.npz: the
seed and actions of profiles/r02_wedged_env.npz) and (b) 32 uniform-random 2v2 envs
x 300 steps, and prints the table.  Test tooling: the oracle in oracle/ is
not modified.
usage: python scripts/toi_repeat_probe.py [--wedged-only] [--json]"""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'gym-ma-survival-2d_amd'))

WEDGED = os.path.join(ROOT, 'tests', 'golden', 'wedged_2v2.npz')
NAMES = ['events', 'repeat', 'repeat_other_static', 'repeat_across_restore', 'calls_ge4', 'events_ge4', 'repeat_ge4']

PATCHES = [
    # per call: the previous event's values
    ("""    sw.alpha0 = 0.0f;
    int valid[ORA_MAX_STAT], count[ORA_MAX_STAT], enabled[ORA_MAX_STAT];""",
     """    sw.alpha0 = 0.0f;
    float prev_[10]; int prev_s_ = -1, have_ = 0, restored_ = 0, ev_ = 0, rep_ = 0;
    int valid[ORA_MAX_STAT], count[ORA_MAX_STAT], enabled[ORA_MAX_STAT];"""),
    # a restored non-event between two events
    ("""            enabled[minS] = 0;
            sw = backup;""",
     """            enabled[minS] = 0;
            restored_ = 1;
            sw = backup;"""),
    # the end of an event
    ("""        sw.c = w->c[i];
        sw.a = w->a[i];
        for (int s = 0; s < ns; ++s) valid[s] = 0;""",
     """        sw.c = w->c[i];
        sw.a = w->a[i];
        {
            float now_[10] = {sw.c0.x, sw.c0.y, sw.a0, sw.c.x, sw.c.y, sw.a, sw.alpha0, w->v[i].x, w->v[i].y, w->w[i]};
            ++ev_;
            if (have_ && memcmp(now_, prev_, sizeof(now_)) == 0) {
                if (prev_s_ != minS) g_rep[2]++;
                else { ++rep_; if (restored_) g_rep[3]++; }
            }
            memcpy(prev_, now_, sizeof(now_));
            prev_s_ = minS; have_ = 1; restored_ = 0;
        }
        for (int s = 0; s < ns; ++s) valid[s] = 0;"""),
    # the end of the call
    ("""    w->c[i] = sw.c;
    w->a[i] = sw.a;
}

void ora_world_step(""",
     """    w->c[i] = sw.c;
    w->a[i] = sw.a;
    g_rep[0] += ev_; g_rep[1] += rep_;
    if (ev_ >= 4) { g_rep[4]++; g_rep[5] += ev_; g_rep[6] += rep_; }
}

void ora_world_step("""),
]
HEADER = """
#include <string.h>
static long long g_rep[8];
void ora_toi_repeat(long long* o, int reset) { for (int k = 0; k < 8; ++k) { o[k] = g_rep[k]; if (reset) g_rep[k] = 0; } }
"""


def build(tmp):
    os.makedirs(os.path.join(tmp, 'oracle'))
    shutil.copytree(os.path.join(ROOT, 'include'), os.path.join(tmp, 'include'))
    for f in os.listdir(os.path.join(ROOT, 'oracle')):
        if f.endswith(('.c', '.h')):
            shutil.copy(os.path.join(ROOT, 'oracle', f), os.path.join(tmp, 'oracle', f))
    path = os.path.join(tmp, 'oracle', 'mas_oracle.c')
    s = open(path).read()
    i = s.index('/* World step: Box2D b2World::Step')
    s = s[:i] + HEADER + s[i:]
    for old, new in PATCHES:
        assert s.count(old) == 1, old[:60]
        s = s.replace(old, new, 1)
    open(path, 'w').write(s)
    so = os.path.join(tmp, 'libtoirep.so')
    subprocess.check_call(['gcc', '-O2', '-std=gnu11', '-fPIC', '-ffp-contract=off', '-shared', '-o', so,
                           path, os.path.join(tmp, 'oracle', 'ora_bench.c'), '-lm', '-lpthread'])
    return so


def probe(wedged_only=False):
    """{'wedged': counts, 'random': counts} (NAMES -> int); 'random' is left
    out with wedged_only."""
    import oracle
    from masurvival.config import NAMED_CONFIGS, ResolvedConfig, pcg64_state
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        oracle.LIB = build(tmp)  # before the first oracle.lib() of the process
        L = oracle.lib()
        L.ora_toi_repeat.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]

        def rd():
            o = (ctypes.c_longlong * 8)()
            L.ora_toi_repeat(o, 1)
            return dict(zip(NAMES, list(o)))
        rc = ResolvedConfig(NAMED_CONFIGS['2v2'])
        d = np.load(WEDGED)
        env = oracle.OracleEnv(rc.to_struct(), pcg64_state(int(d['env_seed'])))
        env.reset()
        rd()
        for t in range(len(d['actions'])):
            if env.step(d['actions'][t])[2]:
                env.reset()
        out['wedged'] = rd()
        if not wedged_only:
            rng = np.random.default_rng(0)
            envs = [oracle.OracleEnv(rc.to_struct(), pcg64_state(s)) for s in range(32)]
            for e in envs:
                e.reset()
            rd()
            for _ in range(300):
                for e in envs:
                    if e.step(rng.integers(0, [3, 3, 3, 2, 2, 2], size=(4, 6)))[2]:
                        e.reset()
            out['random'] = rd()
    return out


def show(tag, c):
    pct = 100 * c['repeat'] / max(c['events'], 1)
    print(f'{tag}: TOI events {c["events"]}; bit-identical to the previous event of the call (same min static) '
          f'{c["repeat"]} ({pct:.0f}%), of which across a restored non-event {c["repeat_across_restore"]}; '
          f'identical with another min static {c["repeat_other_static"]}; SolveTOI calls with >= 4 events '
          f'{c["calls_ge4"]}: events {c["events_ge4"]} ({c["events_ge4"] / max(c["calls_ge4"], 1):.1f} per call), '
          f'repeats {c["repeat_ge4"]} ({c["repeat_ge4"] / max(c["calls_ge4"], 1):.1f} per call)')


def main():
    r = probe('--wedged-only' in sys.argv[1:])
    if '--json' in sys.argv[1:]:
        print(json.dumps(r))
        return
    show('wedged 2v2 env (seed 8754) replayed, 256 steps', r['wedged'])
    if 'random' in r:
        show('32 seeded 2v2 envs x 300 uniform-random steps', r['random'])


if __name__ == '__main__':
    main()
