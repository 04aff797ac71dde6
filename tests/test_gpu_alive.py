"""mas_alive (VecMaSurvival.alive): the agents whose actions the next step
reads, against the observations.  A dead agent's row is zeros apart from its
index and team, so the criterion on an observation is: the last seven columns
of the 'agent' key (health, x, y, angle, vx, vy, omega) are all zero.  An agent
the zone killed in the last step shows health <= 0 with its pose still there:
alive by the criterion and by the mask (it acts once more).

Golden replays at n_envs = 1 check alive() before every step against the
recorded observation the step acts on, with the fixtures' dead-row totals
asserted so that no replay passes on an episode without deaths; a batched
run with auto-reset checks it against the oracle's observations."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import golden_replay as gr  # noqa: E402
from masurvival import abi  # noqa: E402
from gpu_util import class_missing  # noqa: E402
from masurvival.config import C3_CONFIG, ResolvedConfig, pcg64_state  # noqa: E402
from masurvival.vec_env import ShardedVecMaSurvival, VecMaSurvival  # noqa: E402
from oracle import OracleEnv  # noqa: E402

# fixture -> (dead rows, all rows) over the observations its steps act on
GOLDEN = {
    'c1_random_s0.npz': (333, 1108),
    'c3_2v2_script_s3.npz': (418, 1372),
    'ownership_contmelee_s6.npz': (93, 660),
    'nonomni_lastalive_s7.npz': (221, 1264),
    'xxl_ffa8_s17.npz': (1807, 5712),
}


def make_vec(cfg, n, seeds, auto_reset):
    try:
        return VecMaSurvival(cfg, n_envs=n, seeds=seeds, auto_reset=auto_reset)
    except abi.MasError as e:
        class_missing(e)


def alive_of_obs(obs, layout):
    """The criterion on observation rows [..., A, D] (numpy): 1.0 where alive."""
    off, shp = layout['agent']
    ag = obs[..., off:off + shp[0]]
    return (~(ag[..., -7:] == 0).all(-1)).astype(np.float32)


@pytest.mark.parametrize('name', sorted(GOLDEN))
def test_alive_on_golden_replay(name):
    d, cfg = gr.load(name)
    env = make_vec(cfg, 1, [int(d['env_seed'])], False)
    T, A = len(d['done']), env.n_agents
    obs = env.reset().cpu().numpy()[0]
    assert np.array_equal(obs, d['obs'][0])
    acts = torch.as_tensor(d['actions'], device=env.device)
    got = torch.empty((T, 1, A), device=env.device)
    for t in range(T):
        env.alive(out=got[t])
        env.step(acts[t:t + 1])
    got = got.cpu().numpy()[:, 0]
    assert set(np.unique(got)) <= {0.0, 1.0}
    want = alive_of_obs(d['obs'][:T], env.layout)
    bad = np.argwhere(got != want)
    assert bad.size == 0, bad[:10]
    assert (int((want == 0).sum()), T * A) == GOLDEN[name]


def test_alive_batched_autoreset_matches_oracle_observations():
    rc = ResolvedConfig(C3_CONFIG)
    n, T = 128, 300
    seeds = list(range(1000, 1000 + n))
    env = make_vec(C3_CONFIG, n, seeds, True)
    ors = [OracleEnv(rc.to_struct(), pcg64_state(s)) for s in seeds]
    env.reset()
    obs = np.stack([o.reset() for o in ors])
    rng = np.random.default_rng(7)
    got = torch.empty((T + 1, n, rc.n_agents), device=env.device)
    want = np.empty((T + 1, n, rc.n_agents), dtype=np.float32)
    reset_at = np.zeros((T + 1, n), dtype=bool)
    for t in range(T):
        env.alive(out=got[t])
        want[t] = alive_of_obs(obs, env.layout)
        a = rng.integers(0, [3, 3, 3, 2, 2, 2], size=(n, rc.n_agents, 6)).astype(np.int8)
        env.step(torch.as_tensor(a, device=env.device))
        for e in range(n):
            oo, _, dd = ors[e].step(a[e])
            if dd:
                oo = ors[e].reset()
                reset_at[t + 1, e] = True
            obs[e] = oo
    env.alive(out=got[T])
    want[T] = alive_of_obs(obs, env.layout)
    assert np.array_equal(env.obs.cpu().numpy(), obs)  # the two runs are the same trajectories
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, bad[:10]
    dead = want == 0
    assert bool((dead.any(-1) & ~dead.all(-1)).any()), 'no step with dead and alive agents in one env'
    assert reset_at.any(), 'no auto-reset in the run'
    assert bool((got[reset_at] == 1.0).all()), 'an env is not all alive right after its auto-reset'


def test_alive_agrees_with_render_view_and_shards():
    n = 48
    seeds = list(range(300, 300 + n))
    env = make_vec(C3_CONFIG, n, seeds, True)
    try:
        sh = ShardedVecMaSurvival(C3_CONFIG, n_envs=n, shards=3, seeds=seeds, auto_reset=True)
    except abi.MasError as e:
        class_missing(e)
    env.reset()
    sh.reset()
    rng = np.random.default_rng(3)
    mixed = False
    for t in range(200):
        a = torch.as_tensor(rng.integers(0, [3, 3, 3, 2, 2, 2], size=(n, env.n_agents, 6)).astype(np.int8),
                            device=env.device)
        env.step(a)
        sh.step(a)
        if t % 40 == 39:
            al = env.alive()
            assert torch.equal(sh.alive(), al)
            out = torch.full((n, env.n_agents), -1.0, device=env.device)
            assert sh.alive(out=out) is out and torch.equal(out, al)
            al = al.cpu().numpy()
            mixed = mixed or bool((al == 0).any())
            for e in (0, 1, 17, n - 1):
                assert np.array_equal(env.render_view(e)['agents'][:, 3], al[e]), (t, e)
    assert mixed, 'no dead agent at any checked step'


def test_alive_refuses_null_arguments():
    env = make_vec(C3_CONFIG, 4, range(4), True)
    lib = abi.load_library()
    assert lib.mas_alive(env._h, None, None) == -1
    assert lib.mas_last_error().decode().startswith('mas_alive:')
    assert lib.mas_alive(None, ctypes.c_void_p(env.obs.data_ptr()), None) == -1
    with pytest.raises(ValueError):
        env.alive(out=torch.empty((4, env.n_agents), dtype=torch.float64, device=env.device))
