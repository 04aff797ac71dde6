"""What the conservative pre-test of SolveTOI (toi_reject, csrc/mas_physics.h;
DESIGN 4.4.22) may skip: for every b2TimeOfImpact call of world_toi_agent,
would the pre-test at a given margin have rejected it, and what did the call
return?

Builds an INSTRUMENTED COPY of the C oracle in a temp dir.  After each
time_of_impact call of world_toi_agent the copy runs toi_reject (the same
float operations as the device's) on the call's sweep at the margins 0.02
(the old one), 0.002 (MARGIN, the one the kernels use) and 0.0005, and counts
the calls each margin does not reject and -- the soundness check -- the calls
it rejects although the call returned "touching".  For the touching results
it also samples the sweep at 257 points, takes the minimum of the gauge
max(|lx| - ex, |ly| - ey) in the static's frame (refined between the samples
beside the best one: the gauge is convex along the segment, and the touching
time is no sample), and records the largest slack = that minimum - (target +
tolerance): a touching result must sit at or below the threshold, up to the
rounding bound of toi_reject's comment (SLACK_TOL).

Three legs, 2v2: seeded envs on uniform-random actions, the same with each
action held 40 steps (agents push against statics), and the recorded wedged
env (tests/golden/wedged_2v2.npz).  Test tooling: the oracle in oracle/ is
not modified.  Exits 1 if any call that MARGIN rejects returned touching.
usage: python scripts/toi_pretest_probe.py [--envs N] [--steps T] [--json]"""
import argparse
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
MARGINS = (0.02, 0.002, 0.0005)
MARGIN = 0.002  # kToiRejectMargin of csrc/mas_physics.h
SLACK_TOL = 2e-5  # the float rounding bound derived at toi_reject (arena coordinates below 16)
HOLD = 40
HI = [3, 3, 3, 2, 2, 2]

PATCHES = [
    ("""                int st = time_of_impact(&pA, sA, &pB, sw, &beta);
                if (st == TOI_TOUCHING) alpha""",
     """                int st = time_of_impact(&pA, sA, &pB, sw, &beta);
                pretest_probe_(w, s, &sw, st == TOI_TOUCHING);
                if (st == TOI_TOUCHING) alpha"""),
]
HEADER = """
static const float kMargins_[3] = {%s};
static long long g_pt[8];   /* calls, not rejected x3, touching, rejected-but-touching x3 */
static double g_pt_slack = -1e30;  /* largest slack of a touching result */
void ora_toi_pretest(long long* o, double* slack, int reset)
{
    for (int k = 0; k < 8; ++k) { o[k] = g_pt[k]; if (reset) g_pt[k] = 0; }
    *slack = g_pt_slack;
    if (reset) g_pt_slack = -1e30;
}
/* toi_reject of csrc/mas_physics.h, operation for operation, margin given */
static int pretest_reject_(const ora_world* w, int s, v2 p0, v2 p1, float margin)
{
    const float R = b2max(LINEAR_SLOP, POLYGON_RADIUS + w->radius - 3.0f * LINEAR_SLOP) + 0.25f * LINEAR_SLOP + margin;
    v2 l0 = xmult(w->sp[s], w->sq[s], p0), l1 = xmult(w->sp[s], w->sq[s], p1);
    float ex = 0.0f, ey = 0.0f;
    for (int k = 0; k < w->spoly[s].count; ++k) {
        ex = fmaxf(ex, fabsf(w->spoly[s].v[k].x));
        ey = fmaxf(ey, fabsf(w->spoly[s].v[k].y));
    }
    ex += R;
    ey += R;
    if (fminf(l0.x, l1.x) > ex || fmaxf(l0.x, l1.x) < -ex || fminf(l0.y, l1.y) > ey || fmaxf(l0.y, l1.y) < -ey)
        return 1;
    float tmin = 0.0f, tmax = 1.0f;
    v2 d = vsub(l1, l0);
    if (fabsf(d.x) < 1e-12f) {
        if (fabsf(l0.x) > ex) return 1;
    } else {
        float ta = (-ex - l0.x) / d.x, tb = (ex - l0.x) / d.x;
        tmin = fmaxf(tmin, fminf(ta, tb));
        tmax = fminf(tmax, fmaxf(ta, tb));
        if (tmin > tmax) return 1;
    }
    if (fabsf(d.y) < 1e-12f) {
        if (fabsf(l0.y) > ey) return 1;
    } else {
        float ta = (-ey - l0.y) / d.y, tb = (ey - l0.y) / d.y;
        tmin = fmaxf(tmin, fminf(ta, tb));
        tmax = fminf(tmax, fmaxf(ta, tb));
        if (tmin > tmax) return 1;
    }
    return 0;
}
static void pretest_probe_(const ora_world* w, int s, const sweep* sw, int touching)
{
    g_pt[0]++;
    for (int k = 0; k < 3; ++k) {
        if (!pretest_reject_(w, s, sw->c0, sw->c, kMargins_[k])) g_pt[1 + k]++;
        else if (touching) g_pt[5 + k]++;
    }
    if (!touching) return;
    g_pt[4]++;
    /* the gauge along the sweep, in double from the float inputs */
    double ex = 0.0, ey = 0.0;
    for (int k = 0; k < w->spoly[s].count; ++k) {
        ex = fmax(ex, fabs((double)w->spoly[s].v[k].x));
        ey = fmax(ey, fabs((double)w->spoly[s].v[k].y));
    }
    const double qs = w->sq[s].s, qc = w->sq[s].c,
                 thr = (double)b2max(LINEAR_SLOP, POLYGON_RADIUS + w->radius - 3.0f * LINEAR_SLOP)
                       + (double)(0.25f * LINEAR_SLOP);
#define GAUGE_(t, out) do { \
        const double px = (1.0 - (t)) * sw->c0.x + (t) * sw->c.x - w->sp[s].x, \
                     py = (1.0 - (t)) * sw->c0.y + (t) * sw->c.y - w->sp[s].y; \
        const double lx = qc * px + qs * py, ly = -qs * px + qc * py; \
        (out) = fmax(fabs(lx) - ex, fabs(ly) - ey); } while (0)
    double gmin = 1e30;
    int kmin = 0;
    for (int k = 0; k <= 256; ++k) {
        double gk;
        GAUGE_(k / 256.0, gk);
        if (gk < gmin) { gmin = gk; kmin = k; }
    }
    /* the gauge is convex along the segment: its minimum lies beside the best
     * sample; a ternary search there gives it between the samples too (the
     * touching time t1 is no sample) */
    double lo = fmax(0.0, (kmin - 1) / 256.0), hi = fmin(1.0, (kmin + 1) / 256.0);
    for (int it = 0; it < 80; ++it) {
        const double m1 = lo + (hi - lo) / 3.0, m2 = hi - (hi - lo) / 3.0;
        double g1, g2;
        GAUGE_(m1, g1);
        GAUGE_(m2, g2);
        if (g1 < g2) hi = m2; else lo = m1;
        gmin = fmin(gmin, fmin(g1, g2));
    }
#undef GAUGE_
    if (gmin - thr > g_pt_slack) g_pt_slack = gmin - thr;
}
""" % ', '.join('%rf' % m for m in MARGINS)


def build(tmp):
    os.makedirs(os.path.join(tmp, 'oracle'))
    shutil.copytree(os.path.join(ROOT, 'include'), os.path.join(tmp, 'include'))
    for f in os.listdir(os.path.join(ROOT, 'oracle')):
        if f.endswith(('.c', '.h')):
            shutil.copy(os.path.join(ROOT, 'oracle', f), os.path.join(tmp, 'oracle', f))
    path = os.path.join(tmp, 'oracle', 'mas_oracle.c')
    s = open(path).read()
    i = s.index('/* b2World::SolveTOI restricted to one agent')
    s = s[:i] + HEADER + s[i:]
    for old, new in PATCHES:
        assert s.count(old) == 1, old[:60]
        s = s.replace(old, new, 1)
    open(path, 'w').write(s)
    so = os.path.join(tmp, 'libtoipre.so')
    subprocess.check_call(['gcc', '-O2', '-std=gnu11', '-fPIC', '-ffp-contract=off', '-shared', '-o', so,
                           path, os.path.join(tmp, 'oracle', 'ora_bench.c'), '-lm', '-lpthread'])
    return so


def held_actions(rng, t, prev, shape):
    """Uniform-random actions, redrawn every HOLD steps."""
    return rng.integers(0, HI, size=shape) if t % HOLD == 0 else prev


def probe(n_envs=48, steps=400):
    """{'random' | 'held' | 'wedged': {'calls', 'kept' (per margin), 'touching',
    'rejected_touching' (per margin), 'max_touching_slack'}}."""
    import oracle
    from masurvival.config import NAMED_CONFIGS, ResolvedConfig, pcg64_state
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        oracle.LIB = build(tmp)  # before the first oracle.lib() of the process
        L = oracle.lib()
        L.ora_toi_pretest.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double), ctypes.c_int]

        def rd():
            o = (ctypes.c_longlong * 8)()
            sl = ctypes.c_double()
            L.ora_toi_pretest(o, ctypes.byref(sl), 1)
            o = list(o)
            return dict(calls=o[0], kept=o[1:4], touching=o[4], rejected_touching=o[5:8],
                        max_touching_slack=sl.value if o[4] else None)
        rc = ResolvedConfig(NAMED_CONFIGS['2v2'])
        for leg, hold in (('random', False), ('held', True)):
            rng = np.random.default_rng(1 if hold else 0)
            envs = [oracle.OracleEnv(rc.to_struct(), pcg64_state(s)) for s in range(n_envs)]
            for e in envs:
                e.reset()
            rd()
            a = None
            for t in range(steps):
                a = (held_actions(rng, t, a, (n_envs, rc.n_agents, 6)) if hold
                     else rng.integers(0, HI, size=(n_envs, rc.n_agents, 6)))
                for k, e in enumerate(envs):
                    if e.step(a[k])[2]:
                        e.reset()
            out[leg] = rd()
        d = np.load(WEDGED)
        env = oracle.OracleEnv(rc.to_struct(), pcg64_state(int(d['env_seed'])))
        env.reset()
        rd()
        for t in range(len(d['actions'])):
            if env.step(d['actions'][t])[2]:
                env.reset()
        out['wedged'] = rd()
    return out


def unsound(r):
    """Calls that MARGIN rejects although they returned touching, over all legs."""
    return sum(c['rejected_touching'][MARGINS.index(MARGIN)] for c in r.values())


def show(r, n_envs, steps):
    tags = {'random': f'{n_envs} envs x {steps} steps, uniform random each step',
            'held': f'{n_envs} envs x {steps} steps, random, held {HOLD} steps (agents push)',
            'wedged': 'wedged 2v2 env (seed 8754) replayed'}
    print('| actions | TOI calls | ' + ' | '.join(f'not rejected, margin {m}' for m in MARGINS)
          + ' | touching results | ' + ' | '.join(f'rejected but touching, margin {m}' for m in MARGINS)
          + ' | largest slack of a touching result |')
    print('|---' * (6 + 2 * len(MARGINS) - 2) + '|')
    for leg, c in r.items():
        sl = 'n/a' if c['max_touching_slack'] is None else f'{c["max_touching_slack"]:.2e}'
        print(f'| {tags[leg]} | {c["calls"]} | ' + ' | '.join(str(k) for k in c['kept']) + f' | {c["touching"]} | '
              + ' | '.join(str(k) for k in c['rejected_touching']) + f' | {sl} |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=48)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--json', action='store_true')
    args = ap.parse_args()
    r = probe(args.envs, args.steps)
    if args.json:
        print(json.dumps(r))
    else:
        show(r, args.envs, args.steps)
    bad = unsound(r)
    if bad:
        print(f'UNSOUND: margin {MARGIN} rejects {bad} calls that returned touching', file=sys.stderr)
        sys.exit(1)


if __name__ == '__main__':
    main()
