"""Per-kernel instruction-fetch counters of the env-step kernels from rocprofv3
PMC passes of bench.py (each pass a run of its own, --kernel-include-regex
'mas::k_'), over the last `steps` env steps (the timed window):
  pass 1: SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQ_WAVES
  pass 2: SQ_IFETCH SQ_WAIT_INST_ANY SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES
Counters are summed over the chip per dispatch and printed per active wave.
Every launch covers the whole grid; the waves of k_gen_solve_g past the list
and of the slow list's kernels exit at once, so the active waves are
  k_pre_lanes, k_post_lanes<.., 0 / 3>   every launched wave
  k_gen_solve_g (main list)              ceil(general envs / envs per wave)
  slow-list launches (side stream)       `slow_waves`
with the general envs per step from mas_debug_counters (bench.py's result
line, phys_general_envs_last_step).  In a split step the side stream's
launches are dispatched first: the first k_gen_solve_g is the slow list's.
SQC_ICACHE_REQ = HITS + MISSES + MISSES_DUPLICATE: a duplicate is a request
to a line whose miss is already pending, counted apart from the misses.  Two
estimates of the fetch stall per wave, as a share of the wave's cycles
(SQ_WAVE_CYCLES and SQ_WAIT_INST_ANY count units of 4 cycles):
  net   max(0, misses - duplicates) x L2-hit latency
  all   (misses + duplicates) x L2-hit latency: every one of them waits the
        whole latency and none overlaps another wave's issue (an upper bound)
usage: python profiles/icache_summary.py <general_envs> <counter_collection.csv>... [--steps 128] [--epw 8]
       [--slow-waves 1] [--l2-cycles 200]"""
import argparse
import collections
import csv
import re


def kname(full):
    m = re.search(r'mas::(k_\w+)(<[^(]*>)?', full)
    if not m:
        return None
    name, targs = m.group(1), m.group(2) or ''
    if name == 'k_post_lanes':
        sel = re.search(r',\s*(\d+)\s*>$', targs)
        return 'k_post_lanes<%s>' % (sel.group(1) if sel else '-')
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('general_envs', type=float)
    ap.add_argument('csv', nargs='+')
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--epw', type=int, default=8, help='envs per k_gen_solve_g wave (2v2: 8)')
    ap.add_argument('--slow-waves', type=float, default=1.0)
    ap.add_argument('--l2-cycles', type=float, default=200.0)
    args = ap.parse_args()
    gen_waves = -(-args.general_envs // args.epw)
    agg = collections.defaultdict(lambda: collections.defaultdict(float))
    for path in args.csv:
        disp = collections.defaultdict(dict)
        names = {}
        for r in csv.DictReader(open(path)):
            k = kname(r['Kernel_Name'])
            if k is None:
                continue
            d = int(r['Dispatch_Id'])
            disp[d][r['Counter_Name']] = disp[d].get(r['Counter_Name'], 0.0) + float(r['Counter_Value'])
            names[d] = k
        order = sorted(disp)
        starts = [d for d in order if names[d] == 'k_pre_lanes']
        starts = starts[-args.steps:]
        for n, s in enumerate(starts):
            end = starts[n + 1] if n + 1 < len(starts) else order[-1] + 1
            step = [d for d in order if s <= d < end]
            gens = [d for d in step if names[d] == 'k_gen_solve_g']
            # (one launch per world step with MAS_GEN_FUSE2=0 is not handled: the default is one launch)
            label = {d: names[d] for d in step}
            if len(gens) >= 2:
                label[gens[0]] = 'k_gen_solve_g (slow list)'
            for d in gens[-1:]:
                label[d] = 'k_gen_solve_g (main list)'
            for d in step:
                a = agg[(label[d], path)]
                for c, v in disp[d].items():
                    a[c] += v
                a['launches'] += 1
    cols = ['SQC_ICACHE_REQ', 'SQC_ICACHE_HITS', 'SQC_ICACHE_MISSES', 'SQC_ICACHE_MISSES_DUPLICATE', 'SQ_IFETCH',
            'SQ_WAIT_INST_ANY', 'SQ_WAVE_CYCLES', 'SQ_BUSY_CYCLES']
    print('# general envs per step %.0f -> %d active main-list waves; slow-list active waves %.0f; L2-hit %.0f cycles'
          % (args.general_envs, gen_waves, args.slow_waves, args.l2_cycles))
    print('%-28s %8s %9s %9s ' % ('kernel', 'launches', 'waves/l', 'active/l')
          + ' '.join('%11s' % c.replace('SQC_ICACHE_', 'IC_').replace('SQ_', '').replace('MISSES_DUPLICATE', 'MISS_DUP')
                     for c in cols) + '   net_stall share  all_stall share   (cycles per active wave)')
    for k in sorted(set(kp[0] for kp in agg)):
        # per active wave, each counter from the first pass that has it (the
        # passes are separate runs: their launch counts may differ slightly)
        per = {}
        launches = wl = act = 0.0
        for path in args.csv:
            a = agg.get((k, path))
            if not a:
                continue
            n = a['launches']
            w = a['SQ_WAVES'] / n
            if 'slow list' in k or k == 'k_post_lanes<2>':
                ac = args.slow_waves
            elif 'main list' in k:
                ac = gen_waves
            else:
                ac = w
            if not launches:
                launches, wl, act = n, w, ac
            for c in cols:
                if c in a and c not in per:
                    per[c] = a[c] / (ac * n)
        mis, dup = per.get('SQC_ICACHE_MISSES', 0.0), per.get('SQC_ICACHE_MISSES_DUPLICATE', 0.0)
        net, tot = max(0.0, mis - dup) * args.l2_cycles, (mis + dup) * args.l2_cycles
        wc = 4.0 * per.get('SQ_WAVE_CYCLES', 0.0)
        print('%-28s %8d %9.0f %9.0f ' % (k, launches, wl, act)
              + ' '.join('%11.0f' % per.get(c, float('nan')) for c in cols)
              + ' %11.0f %5.1f%% %10.0f %5.1f%%' % (net, 100.0 * net / wc if wc else float('nan'),
                                                   tot, 100.0 * tot / wc if wc else float('nan')))


if __name__ == '__main__':
    main()
