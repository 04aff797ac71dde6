"""The HIP env step against the fp64 reference of the rules' geometry
(tests/rules_ref.py, tests/rules_laws.py; the same laws, bands and coverage
floors as tests/test_rules_reference.py applies to the C oracle): who sees
whom, whom a swing hits, which item is picked up, who stands outside the zone.

Per scenario two VecMaSurvival instances of 128 envs, the config with
observation.omniscent True and False on the same seeds, run 200 steps with
auto-reset on the same actions, which the controller computes on the host from
the omniscient twin's rows.  On top of the shared laws:

  * a sample of envs of the non-omniscient twin (the first and last, both
    sides of the 64 boundary, 8 random) is replayed through the oracle with
    the recorded actions: np.array_equal on every observation float, reward and
    done flag, resets included, which carries the bit-exact bar of the
    non-omniscient camera pass to hiding, foraging and brawling trajectories
    that uniform-random actions do not produce;
  * no list overflowed, no action was out of range."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import golden_replay as gr  # noqa: E402
import rules_laws as rl  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival import abi  # noqa: E402
from masurvival.config import ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402

N_ENVS, N_STEPS = 128, 200


def _sample(n, seed):
    fixed = [e for e in (0, 1, 63, 64, n - 1) if e < n]
    rest = [e for e in range(n) if e not in fixed]
    return sorted(fixed + np.random.default_rng(seed).choice(rest, size=8, replace=False).tolist())


@pytest.mark.parametrize('name', rl.SCENARIOS)
def test_kernels_obey_the_rules_and_match_the_oracle(name):
    sc = rl.scenario(name)
    n = N_ENVS
    cfgs = rl.twin_configs(sc.cfg)
    try:
        envs = [VecMaSurvival(c, n_envs=n, seeds=range(n), auto_reset=True) for c in cfgs]
    except abi.MasError as e:
        class_missing(e)
    sample = _sample(n, len(name))
    rec, obs0 = [], []

    def reset():
        o = tuple(e.reset().cpu().numpy() for e in envs)
        obs0.append(o[1])
        return o

    def step(a):
        out = []
        for e in envs:
            o, r, dn, _ = e.step(torch.as_tensor(a, device=e.device))
            out.append((o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy().astype(bool)))
        return out

    def record(t, a, non):
        o, r, dn = non
        rec.append((a[sample].copy(), o[sample].copy(), r[sample].copy(), dn[sample].copy()))

    st = rl.run(sc, reset, step, range(n), N_STEPS, record=record)
    guards = [e.debug_guards() for e in envs]
    invalid = [e.invalid_actions() for e in envs]
    for e in envs:
        e.close()
    print(name, st.report())
    rl.check(sc, st)
    assert all(g['list_overflow'] == 0 for g in guards) and invalid == [0, 0], (guards, invalid)

    # the sampled envs of the non-omniscient twin again, through the oracle
    rc = ResolvedConfig(cfgs[1])
    assert not rc.to_struct().omniscient
    for k, e in enumerate(sample):
        ora = OracleEnv(rc.to_struct(), pcg64_state(e))
        assert np.array_equal(obs0[0][e], ora.reset()), (name, e)
        for t, (a, o, r, dn) in enumerate(rec):
            oo, rr_, dd = ora.step(a[k])
            if dd:
                oo = ora.reset()
            assert bool(dn[k]) == dd and np.array_equal(r[k], rr_), (name, t, e)
            assert np.array_equal(o[k], oo), (name, t, e, gr.diff(o[k], oo))
