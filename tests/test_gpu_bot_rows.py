"""mas_bot_act row by row against tests/bot_ref.py (fp64, written from the
header's text): exact outside the near rows (a comparison within 1e-4 of its
threshold), which may be at most 0.5 % of the rows of a call and are counted in
the assert messages.  Synthetic rows (tests/bot_rows.py) over seven configs,
every kind, n_envs 1..1000, three masks and two strides; hand-made edge rows
(exact ties, thresholds met exactly) compared on every row, near or not; and
200 steps of rows recorded from a 2v2 x 64 env the bots themselves drive."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import bot_ref  # noqa: E402
import bot_rows  # noqa: E402
from masurvival.bots import BOT_KINDS, bot_act  # noqa: E402
from masurvival.config import C1_CONFIG, C3_CONFIG, C5_CONFIG, ResolvedConfig  # noqa: E402

SEED = 20
NEAR_CAP = 0.005
N_ENVS = (1, 63, 64, 65, 1000)
_MELEE = {'melee': {'range': 2, 'damage': 20, 'cooldown': 40, 'drift': True}}
CONFIGS = {
    '1v1': C1_CONFIG,
    '2v2_teams': C3_CONFIG,
    'ffa4_16_heals': C5_CONFIG,
    '3_agents': dict(_MELEE, agents={'n_agents': 3, 'agent_size': 1}),
    '6_agents_xl': dict(_MELEE, agents={'n_agents': 6, 'agent_size': 1}, teams={'twoteams': True}),
    '8_agents_xxl': dict(_MELEE, agents={'n_agents': 8, 'agent_size': 1}, teams={'twoteams': True},
                         spawn_grid={'grid_size': 8, 'floor_size': 20},
                         heals={'reset_spawns': {'n_items': 16, 'item_size': 0.5}, 'heal': {'healing': 50}}),
    'no_heals': dict(_MELEE, agents={'n_agents': 4, 'agent_size': 1},
                     heals={'reset_spawns': {'n_items': 0, 'item_size': 0.5}, 'heal': {'healing': 50}}),
}
FILL = 9  # what the action bytes hold before a call


def _masks(A):
    return {'single': 1 << (A - 1), 'alternating': sum(1 << a for a in range(0, A, 2)), 'all': (1 << A) - 1}


def _selected(mask, A, n_envs):
    return np.tile(np.array([(mask >> a) & 1 for a in range(A)], dtype=bool), n_envs)


@pytest.fixture(scope='module')
def batches():
    """Per config: the struct, the 1000-env rows at both strides on the device
    (the same columns below obs_dim), and the reference per kind, computed once."""
    out = {}
    for name, cfg in CONFIGS.items():
        cs = ResolvedConfig(cfg).to_struct()
        D, _ = bot_rows.layout_of(cs)
        rows = bot_rows.random_rows(cs, max(N_ENVS), SEED)
        wide = np.full((rows.shape[0], bot_rows.stride_of(D, wider=True)), bot_rows.SENTINEL, dtype=np.float32)
        wide[:, :D] = rows[:, :D]
        ref = {k: bot_ref.bot_ref(k, rows, cs) for k in BOT_KINDS.values()}
        dev = [torch.from_numpy(r).to(torch.bfloat16).cuda() for r in (rows, wide)]
        for r, d in zip((rows, wide), dev):
            assert np.array_equal(d.float().cpu().numpy(), r)  # the rows were bf16-exact
        out[name] = (cs, dev, ref)
    return out


def _run(cs, kind, x, n_envs, mask):
    A = int(cs.n_agents)
    acts = torch.full((n_envs * A, 6), FILL, dtype=torch.int8, device=x.device)
    bot_act(cs, kind, x[:n_envs * A], A, mask, acts)
    return acts.cpu().numpy()


def _compare(got, want, near, sel, what):
    n_near = int((near & sel).sum())
    bad = (got != want).any(axis=1) & sel & ~near
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {int(sel.sum())} selected rows differ outside the '
                           f'{n_near} near rows; first {int(np.flatnonzero(bad)[0])}: kernel '
                           f'{got[bad][0].tolist()} reference {want[bad][0].tolist()}')
    assert n_near <= NEAR_CAP * int(sel.sum()), f'{what}: {n_near} near rows of {int(sel.sum())} selected'
    assert (got[~sel] == FILL).all(), f'{what}: an unselected row was written'
    # near rows too hold valid actions
    assert (got[sel] >= 0).all() and (got[sel][:, :3] <= 2).all() and (got[sel][:, 3:] <= 1).all(), what


@pytest.mark.parametrize('kind', list(BOT_KINDS))
@pytest.mark.parametrize('config', list(CONFIGS))
def test_rows_equal_the_reference(batches, config, kind):
    cs, dev, ref = batches[config]
    A = int(cs.n_agents)
    want, near = ref[BOT_KINDS[kind]]
    for n in N_ENVS:
        for mname, mask in _masks(A).items():
            sel = _selected(mask, A, n)
            for x, sname in zip(dev, ('stride Dx', 'wider stride')):
                got = _run(cs, kind, x, n, mask)
                _compare(got, want[:n * A], near[:n * A], sel, f'{config} {kind} n_envs {n} mask {mname} {sname}')


def test_the_rule_acts(batches):
    """The synthetic rows reach every action value the rule can give."""
    cs, dev, ref = batches['2v2_teams']
    got = _run(cs, 'forager', dev[0], 1000, 0b1111)
    hun = _run(cs, 'hunter', dev[0], 1000, 0b1111)
    assert set(np.unique(hun[:, 0])) == {1, 2} and set(np.unique(hun[:, 2])) == {0, 1, 2}
    assert set(np.unique(hun[:, 3])) == {0, 1} and set(np.unique(got[:, 4])) == {0, 1}
    assert (got != hun).any()
    idle = _run(cs, 'idle', dev[0], 1000, 0b1111)
    assert (idle == np.array([1, 1, 1, 0, 0, 0], dtype=np.int8)).all()


def test_columns_past_obs_dim_are_never_read_and_calls_repeat(batches):
    for config in ('2v2_teams', '8_agents_xxl', '1v1'):
        cs, dev, _ = batches[config]
        A = int(cs.n_agents)
        D, _ = bot_rows.layout_of(cs)
        for x in dev:
            for kind in ('hunter', 'forager'):
                first = _run(cs, kind, x, 1000, (1 << A) - 1)
                assert np.array_equal(first, _run(cs, kind, x, 1000, (1 << A) - 1))  # the same call twice
                y = x.clone()
                y[:, D:] = float('nan')
                assert np.array_equal(first, _run(cs, kind, y, 1000, (1 << A) - 1)), (config, kind)


@pytest.mark.parametrize('kind', ['hunter', 'forager'])
def test_edge_rows_are_exact_on_every_row(kind):
    """Ties, a target at the own position and thresholds met exactly: numbers
    with a few bits and the heading 0, so fp32 and fp64 agree to the bit and the
    near flag is not consulted."""
    cs = ResolvedConfig(C3_CONFIG).to_struct()
    rows, labels = bot_rows.edge_rows(cs)
    want, _ = bot_ref.bot_ref(BOT_KINDS[kind], rows, cs)
    x = torch.from_numpy(rows).to(torch.bfloat16).cuda()
    got = _run(cs, kind, x, len(labels), 0b1111)
    for i, label in enumerate(labels):
        assert got[4 * i].tolist() == want[4 * i].tolist(), (kind, label)
    assert np.array_equal(got, want)
    # what some of them must give, whatever the reference says
    row = {label: got[4 * i].tolist() for i, label in enumerate(labels)}
    assert row['dead self'] == [1, 1, 1, 0, 0, 0]
    assert row['nothing in sight'] == [1, 1, 2, 0, 0, 0]
    assert row['use at exactly the threshold'][4] == 1 and row['no use one above the threshold'][4] == 0
    if kind == 'hunter':
        assert row['mirrored enemies: the lower index'] == [2, 1, 2, 0, 0, 0]   # (4, 3): ahead, to the left
        assert row['mirrored enemies, order swapped'] == [1, 1, 0, 0, 0, 0]     # (-2, 1): behind, to the right
        assert row['enemy at exactly the reach'] == [2, 1, 1, 1, 0, 0]
        assert row['enemy just past the reach'] == [2, 1, 1, 0, 0, 0]
        assert row['enemy at exactly the standoff'] == [1, 1, 1, 1, 0, 0]
    else:
        assert row['enemy at exactly 4 m'][0] == 2 and row['enemy at 4.25 m'] == [1, 1, 2, 0, 0, 0]


def test_recorded_rows_of_an_env_the_bots_drive():
    from masurvival.vec_env import VecMaSurvival
    N, T = 64, 200
    env = VecMaSurvival(C3_CONFIG, n_envs=N, seeds=range(N), auto_reset=True)
    assert env.supports_step_x()
    cs, A, D = env.rc.to_struct(), env.n_agents, env.obs_dim
    Dx = bot_rows.stride_of(D)
    xs = torch.zeros((T + 1, N * A, Dx), dtype=torch.bfloat16, device=env.device)
    xs[0, :, :D].copy_(env.reset().reshape(N * A, D))
    acts = torch.zeros((T, N, A, 6), dtype=torch.int8, device=env.device)
    r = torch.empty((N, A), device=env.device)
    d = torch.empty((N,), dtype=torch.uint8, device=env.device)
    for t in range(T):
        bot_act(cs, 'hunter', xs[t], A, 0b0011, acts[t].view(-1, 6))
        bot_act(cs, 'forager', xs[t], A, 0b1100, acts[t].view(-1, 6))
        env.step_x(acts[t], xs[t + 1], r, d)
    rows = xs[:T].float().cpu().numpy().reshape(T * N * A, Dx)
    got = acts.cpu().numpy().reshape(T * N * A, 6)
    env.close()
    for kind, mask in (('hunter', 0b0011), ('forager', 0b1100)):
        want, near = bot_ref.bot_ref(BOT_KINDS[kind], rows, cs)
        sel = _selected(mask, A, T * N)
        n_near = int((near & sel).sum())
        bad = (got != want).any(axis=1) & sel & ~near
        assert not bad.any(), f'{kind}: {int(bad.sum())} rows differ outside the {n_near} near rows'
        assert n_near <= NEAR_CAP * int(sel.sum()), f'{kind}: {n_near} near rows of {int(sel.sum())}'
    assert (got[:, 0] == 2).any() and (got[:, 3] == 1).any()  # they moved and fought
