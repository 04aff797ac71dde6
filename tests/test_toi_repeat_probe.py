"""What the repeated-event skip of toi_agent_group (csrc/mas_physics.h) relies
on, measured on the C oracle by scripts/toi_repeat_probe.py (an instrumented
temp copy; its own process, so this one's oracle library stays the real one):
in the recorded wedged 2v2 env most TOI events of a capped SolveTOI call leave
the sweep, v and w bit for bit as the event before them did, and always with
the same min static."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wedged_replay_repeats_most_toi_events():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, 'scripts', 'toi_repeat_probe.py'),
                                   '--wedged-only', '--json'], text=True)
    c = json.loads(out.strip().splitlines()[-1])['wedged']
    print(c)
    assert c['calls_ge4'] > 0 and c['events_ge4'] >= 4 * c['calls_ge4'], c
    # repeats are at least half of the events of the calls with >= 4 events
    assert 2 * c['repeat_ge4'] >= c['events_ge4'], c
    # an identical event never comes with another min static than the previous event's
    assert c['repeat_other_static'] == 0, c
