"""bench.py --dump-outputs DIR: a plain run (no --full) writes what the timed
window's last step computed as float32 .npy files, the same from run to run
for the same arguments, and its result line carries the timed step count and
ms_per_step with the --full extras (CPU baseline, measured traffic) absent."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, D, H, STEPS = 512, 4, 160, 4, 8
ARGS = ['--gpus', '1', '--envs', str(N), '--steps', str(STEPS), '--warmup', '2', '--horizon', str(H)]
SHAPES = {'actions': (N, A, 6), 'logp': (N, A), 'values': (N, A), 'rewards': (N, A), 'dones': (N,),
          'next_obs': (N, A, D), 'bootstrap_values': (N, A), 'advantages': (H, N, A), 'returns': (H, N, A),
          'policy_params': None, 'update_stats': (5,)}


def _run(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *ARGS, '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


@pytest.fixture(scope='module')
def first(tmp_path_factory):
    return _run(tmp_path_factory.mktemp('dump_a'))


def test_plain_run_line_and_dumped_arrays(first):
    line, arrs = first
    assert line['steps'] == STEPS and line['n_gpus'] == 1 and line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(N * A * STEPS / (line['ms_per_step'] * 1e-3 * STEPS))
    assert line['config']['updates_in_timed_region'] == STEPS // H
    assert line['cpu_baseline'] is None and line['roofline']['traffic'] is None
    assert 'traffic_live' not in line['roofline']
    assert set(arrs) == set(SHAPES)
    for k, v in arrs.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        if SHAPES[k] is not None:
            assert v.shape == SHAPES[k], (k, v.shape)
    assert sum(v.nbytes for v in arrs.values()) <= 64 << 20
    assert arrs['policy_params'].ndim == 1 and arrs['policy_params'].size > 256 * 256
    a = arrs['actions']
    assert (a == np.round(a)).all() and a.min() >= 0 and (a.reshape(-1, 6).max(0) <= [2, 2, 2, 1, 1, 1]).all()
    assert np.abs(arrs['next_obs']).max() > 0 and np.abs(arrs['advantages']).max() > 0


def test_second_run_dumps_the_same_arrays(first, tmp_path):
    _, again = _run(tmp_path)
    for k, v in first[1].items():
        assert np.array_equal(v, again[k]), k
