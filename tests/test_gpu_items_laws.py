"""The HIP env step against the fp64 item ledger (tests/items_ref.py,
tests/items_laws.py; the same laws, tolerances, caps and coverage floors as
tests/test_items_reference.py applies to the C oracle): the world a reset
deals, placing a box, give, the tops of the inventories, conservation, death
drops and box ownership.

Per scenario one omniscient VecMaSurvival of 128 envs runs 200 steps with
auto-reset on actions the controller computes on the host from its rows; the
`ffal` capacity class (8 slots, 24 heals, 16 owned boxes) runs the loot
scenario at 64 envs.  On top of the shared laws:

  * a sample of envs (the first and last, both sides of the 64 boundary, 8
    random) and every env in which the ledger saw a spawn refused (an env
    already at n_boxes / n_heals, which only the copies of double pickups
    reach) is replayed through the oracle with the recorded actions:
    np.array_equal on every observation float, reward and done flag, resets
    included, which carries the bit-exact bar to handover, building and
    looting trajectories that uniform-random actions do not produce;
  * no list overflowed, no action was out of range, and the device refused
    as many spawns as the ledger counted (at least as many where the ledger
    could not judge every env-step).

loot_ffal runs the capacity suite's config as it is: its zone ends the episodes
before the stacks grow beyond depth 3 or 4 of 8, so the heal and item lists are
at their limits there, the stacks are not."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import golden_replay as gr  # noqa: E402
import items_laws as il  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival import abi  # noqa: E402
from masurvival.config import ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_rules_laws import _sample  # noqa: E402

N_STEPS = 200
CASES = [(name, 128) for name in il.SCENARIOS] + [('loot_ffal', 64)]


@pytest.mark.parametrize('name,n', CASES)
def test_kernels_obey_the_item_laws_and_match_the_oracle(name, n):
    sc = il.scenario(name)
    try:
        env = VecMaSurvival(sc.cfg, n_envs=n, seeds=range(n), auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    sample = _sample(n, len(name))
    rec, obs0 = [], []   # every env's actions and rows: the envs to replay are known only at the end

    def reset():
        obs0.append(env.reset().cpu().numpy())
        return obs0[0]

    def step(a):
        o, r, dn, _ = env.step(torch.as_tensor(a, device=env.device))
        return o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy().astype(bool)

    def record(t, a, o, r, dn):
        rec.append((a.copy(), o.copy(), r.copy(), dn.copy()))

    st = il.run(sc, reset, step, range(n), N_STEPS, record=record)
    guards, invalid, refused = env.debug_guards(), env.invalid_actions(), env.spawn_refused()
    env.close()
    print(name, st.report())
    il.check(sc, st)
    assert guards['list_overflow'] == 0 and invalid == 0, (guards, invalid)
    counted = st.count.get('spawn_refused', 0)
    assert refused >= counted and (refused == counted or st.count.get('conserve_skipped', 0) > 0), (refused, counted)
    sample = sorted(set(sample) | set(st.refused_envs))

    # the sampled envs again, through the oracle
    rc = ResolvedConfig(sc.cfg)
    assert rc.to_struct().omniscient
    for e in sample:
        ora = OracleEnv(rc.to_struct(), pcg64_state(e))
        assert np.array_equal(obs0[0][e], ora.reset()), (name, e)
        for t, (a, o, r, dn) in enumerate(rec):
            oo, rr_, dd = ora.step(a[e])
            if dd:
                oo = ora.reset()
            assert bool(dn[e]) == dd and np.array_equal(r[e], rr_), (name, t, e)
            assert np.array_equal(o[e], oo), (name, t, e, gr.diff(o[e], oo))


def test_loot_ffal_is_the_capacity_suites_config():
    from test_gpu_capacity import TEAMS_BIG
    assert il.TEAMS_BIG == TEAMS_BIG
