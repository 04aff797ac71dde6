"""What the margin of toi_reject (csrc/mas_physics.h) relies on, measured on
the C oracle by scripts/toi_pretest_probe.py (an instrumented temp copy; its
own process, so this one's oracle library stays the real one): no
b2TimeOfImpact call that the pre-test rejects returns "touching", every
touching result sits at or below target + tolerance in the gauge the pre-test
uses (up to the rounding bound its comment derives), and the margin removes most of the calls the old 0.02 let through."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def test_script_margin_is_the_kernels_margin():
    import toi_pretest_probe as probe
    src = open(os.path.join(ROOT, 'gym-ma-survival-2d_amd', 'csrc', 'mas_physics.h')).read()
    m = re.search(r'kToiRejectMargin\s*=\s*([0-9.eE+-]+)f\s*;', src)
    assert m and float(m.group(1)) == probe.MARGIN and probe.MARGIN in probe.MARGINS, m


def test_rejected_calls_never_touch():
    import toi_pretest_probe as probe
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'toi_pretest_probe.py'),
                        '--envs', '6', '--steps', '100', '--json'], text=True, stdout=subprocess.PIPE)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print(r)
    assert p.returncode == 0  # the script's own soundness check
    assert set(r) == {'random', 'held', 'wedged'}
    for leg, c in r.items():
        # sound at every margin probed, the old one included
        assert c['rejected_touching'] == [0, 0, 0], (leg, c)
        # a tighter margin keeps a subset; touching calls are never rejected
        assert c['calls'] >= c['kept'][0] >= c['kept'][1] >= c['kept'][2] >= c['touching'], (leg, c)
        # a touching result's sweep reaches the threshold in the pre-test's
        # gauge (the exact minimum over the segment, not only the samples), up
        # to the float rounding of both sides: the bound derived at toi_reject
        if c['touching']:
            assert c['max_touching_slack'] <= probe.SLACK_TOL, (leg, c)
    # the legs exercise it: touching results exist, and the pushing agents'
    # resting contacts are what the tighter margin removes
    assert r['held']['touching'] > 0 and r['wedged']['touching'] > 0
    assert 4 * r['held']['kept'][1] < r['held']['kept'][0], r['held']
