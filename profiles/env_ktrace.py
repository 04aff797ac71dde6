"""Per-kernel time of the env step from a rocprofv3 --kernel-trace run of
bench.py, over the last `steps` env steps (the timed window): mean / p50 /
p90 / max of k_pre_lanes, k_gen_solve_g and k_post_lanes, and the launch
group's span (k_pre_lanes start to the last env kernel's end).  In a split
step the side stream's launches (the slow list's: one or a few active waves)
are dispatched before the caller's stream's, so the first k_gen_solve_g /
k_post_lanes dispatch of the step is the slow list's.
usage: python profiles/env_ktrace.py <run_kernel_trace.csv>... [--steps 128]"""
import csv
import re
import sys

import numpy as np


def steps_of(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    steps, cur = [], None
    for r in rows:
        m = re.search(r'mas::(k_pre_lanes|k_gen_solve_g|k_post_lanes)<', r['Kernel_Name'])
        if not m:
            continue
        if m.group(1) == 'k_pre_lanes':
            cur = {'t0': int(r['Start_Timestamp']), 'end': 0, 'k': {}}
            steps.append(cur)
        if cur is None:
            continue
        cur['k'].setdefault(m.group(1), []).append((int(r['Dispatch_Id']),
                                                    (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
        cur['end'] = max(cur['end'], int(r['End_Timestamp']))
    for s in steps:
        s['k'] = {k: [d for _, d in sorted(v)] for k, v in s['k'].items()}
    return steps


def main():
    args = sys.argv[1:]
    n = 128
    if '--steps' in args:
        i = args.index('--steps')
        n = int(args[i + 1])
        del args[i:i + 2]
    for path in args:
        st = steps_of(path)[-n:]
        split = [s for s in st if len(s['k'].get('k_post_lanes', [])) > 1]
        print(f'{path}: {len(st)} steps, {len(split)} split (us: calls mean p50 p90 max)')
        fam = {'k_pre_lanes': [s['k']['k_pre_lanes'][0] for s in st],
               'k_gen_solve_g (main list)': [s['k']['k_gen_solve_g'][-1] for s in st if 'k_gen_solve_g' in s['k']],
               'k_gen_solve_g (slow list)': [s['k']['k_gen_solve_g'][0] for s in split if len(s['k']['k_gen_solve_g']) > 1],
               'k_post_lanes (all envs)': [s['k']['k_post_lanes'][0] for s in st if len(s['k'].get('k_post_lanes', [])) == 1],
               'k_post_lanes (main envs)': [s['k']['k_post_lanes'][-1] for s in split],
               'k_post_lanes (slow list)': [s['k']['k_post_lanes'][0] for s in split],
               'span': [(s['end'] - s['t0']) / 1e3 for s in st],
               'span, split steps': [(s['end'] - s['t0']) / 1e3 for s in split],
               'span, one-stream steps': [(s['end'] - s['t0']) / 1e3 for s in st if s not in split]}
        for k, v in fam.items():
            if not v:
                continue
            v = np.array(v)
            print(f'  {k:28s} {len(v):5d} {v.mean():8.1f} {np.percentile(v, 50):8.1f} {np.percentile(v, 90):8.1f} {v.max():8.1f}')


if __name__ == '__main__':
    main()
