"""The HIP env step against fp64 closed forms and invariants, on trajectories
driven into contact (tests/physics_laws.py; the same laws, tolerances and
coverage floors as tests/test_physics_reference.py applies to the C oracle).

Per scenario 256 envs (ffa4_lidar: 64) run 300 (80) steps with auto-reset;
the controller computes every step's actions on the host from the GPU's own
rows.  On top of the shared laws:

  * law 2: every env whose gen_flags() byte is 0 after a step (the kernels
    took their contact-free fast path) follows the free-flight closed form for
    all its alive agents, with no "in contact" filter: the fast-path
    classifier is tied to physics, not to the oracle;
  * both paths are taken in every scenario, the per-env TOI counter moves in
    bare_walls, no list overflowed, no action was out of range;
  * a sample of envs (the first and last, both sides of the 64 and 128
    boundaries, 8 random) is replayed through the oracle with the recorded
    actions: np.array_equal on every observation float, reward and done flag,
    which extends the bit-exact bar to contact-heavy trajectories."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import golden_replay as gr  # noqa: E402
import physics_laws as pl  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival import abi  # noqa: E402
from masurvival.config import ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402

N_ENVS, N_STEPS = 256, 300
LIDAR_ENVS, LIDAR_STEPS = 64, 80


def _sample(n, seed):
    fixed = [e for e in (0, 1, 63, 64, 127, 128, 255) if e < n]
    rest = [e for e in range(n) if e not in fixed]
    return sorted(fixed + np.random.default_rng(seed).choice(rest, size=8, replace=False).tolist())


@pytest.mark.parametrize('name', pl.SCENARIOS)
def test_kernels_obey_the_laws_and_match_the_oracle_in_contact(name):
    sc = pl.scenario(name)
    n, T = (LIDAR_ENVS, LIDAR_STEPS) if sc.lidar_only else (N_ENVS, N_STEPS)
    try:
        env = VecMaSurvival(sc.cfg, n_envs=n, seeds=range(n), auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    toi_cnt = torch.zeros((n,), dtype=torch.int32, device=env.device)
    env.set_toi_counter(toi_cnt)
    sample = _sample(n, len(name))
    rec = []

    def step(a):
        o, r, dn, _ = env.step(torch.as_tensor(a, device=env.device))
        return o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy().astype(bool)

    def record(t, a, o, r, dn):
        rec.append((a[sample].copy(), o[sample].copy(), r[sample].copy(), dn[sample].copy()))

    obs0 = []
    st = pl.run(sc, lambda: obs0.append(env.reset().cpu().numpy()) or obs0[0], step, range(n), T,
                gen_flags=lambda: env.gen_flags().cpu().numpy(), record=record)
    toi = toi_cnt.cpu().numpy()
    env.set_toi_counter(None)
    guards, invalid = env.debug_guards(), env.invalid_actions()
    env.close()
    print(name, st.report(), 'TOI events', int((toi & 0xffff).sum()))
    pl.check(sc, st)
    assert st.count['fast_env_steps'] > 0 and st.count['general_env_steps'] > 0, st.report()
    assert guards['list_overflow'] == 0 and invalid == 0, (guards, invalid)
    if name == 'bare_walls':
        assert (toi & 0xffff).sum() > 0

    # the sampled envs again, through the oracle
    rc = ResolvedConfig(sc.cfg)
    for k, e in enumerate(sample):
        ora = OracleEnv(rc.to_struct(), pcg64_state(e))
        assert np.array_equal(obs0[0][e], ora.reset()), (name, e)
        for t, (a, o, r, dn) in enumerate(rec):
            oo, rr, dd = ora.step(a[k])
            if dd:
                oo = ora.reset()
            assert bool(dn[k]) == dd and np.array_equal(r[k], rr), (name, t, e)
            assert np.array_equal(o[k], oo), (name, t, e, gr.diff(o[k], oo))
