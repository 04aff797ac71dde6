"""The scripted bots' rule on the CPU oracle: tests/bot_ref.py (fp64 numpy,
written from the header's text) plays 32 seeds per pairing on bf16-rounded
rows, and masurvival.bots.bot_actions_reference must agree with it on every
row outside the near band.  The bars are conditions the rule has to meet, not
measurements; the measured shares are in profiles/bots.txt."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import bot_play  # noqa: E402
import bot_ref  # noqa: E402
from masurvival.bots import BOT_KINDS, bot_actions_reference  # noqa: E402
from masurvival.config import C5_CONFIG, ResolvedConfig  # noqa: E402

NEAR_CAP = 0.005


@pytest.fixture(scope='module')
def games():
    return bot_play.play_all()


@pytest.mark.parametrize('config', list(bot_play.CONFIGS))
def test_hunter_beats_idle_in_more_than_half_of_the_episodes(games, config):
    r = games[config, ('hunter', 'idle')]
    assert r['finished'] == r['episodes'] == 32
    assert 2 * r['wins'][0] > r['episodes'], r


@pytest.mark.parametrize('config', list(bot_play.CONFIGS))
def test_forager_uses_heals_and_lives_no_shorter_than_idle(games, config):
    idle = games[config, ('idle', 'idle')]
    assert idle['heal_used'] == 0
    for pair in (('forager', 'idle'), ('hunter', 'forager')):
        r = games[config, pair]
        assert r['heal_used'] >= 1, (pair, r)
    r = games[config, ('forager', 'idle')]
    assert r['mean_length'] >= idle['mean_length'], (r, idle)


@pytest.mark.parametrize('config', list(bot_play.CONFIGS))
def test_hunter_against_forager_finishes_every_episode(games, config):
    r = games[config, ('hunter', 'forager')]
    assert r['finished'] == r['episodes'] == 32, r


def test_reference_equals_bot_ref_outside_near_rows_and_near_rows_are_rare(games):
    for key, r in games.items():
        assert r['rows'] > 0
        assert r['mismatch'] == 0, (key, r)
        assert r['near'] <= NEAR_CAP * r['rows'], f'{key}: {r["near"]} near rows of {r["rows"]}'


def test_kinds_agree_between_the_modules():
    assert bot_ref.KINDS == BOT_KINDS
    assert (bot_ref.IDLE, bot_ref.HUNTER, bot_ref.FORAGER) == (0, 1, 2)


def test_reference_shapes_dtypes_and_idle():
    rc = ResolvedConfig(C5_CONFIG)  # FFA4, 16 heals, no teams
    D = 8 + 6 + 3 * 8 + 3 + 16 * 2 + 16 + 2 + 16 * 11 + 16 + 16 * 10 + 16 + 8 + 1
    g = torch.Generator().manual_seed(0)
    obs = torch.randn((5, 4, D), generator=g).to(torch.bfloat16)
    for kind in ('idle', 'hunter', 'forager', 'bot:forager', 2):
        a = bot_actions_reference(kind, obs, rc)
        assert a.shape == (5, 4, 6) and a.dtype == torch.int8
        assert bool((a[..., 1] == 1).all()) and bool((a[..., 5] == 0).all())
        assert int(a.min()) >= 0 and bool((a[..., :3] <= 2).all()) and bool((a[..., 3:] <= 1).all())
        k = kind if isinstance(kind, int) else BOT_KINDS[kind.replace('bot:', '')]
        want, nr = bot_ref.bot_ref(k, obs.float().numpy().reshape(20, D), rc.to_struct())
        assert np.array_equal(a.numpy().reshape(20, 6)[~nr], want[~nr])
    idle = bot_actions_reference('idle', obs, rc)
    assert torch.equal(idle, torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.int8).expand(5, 4, 6))
    with pytest.raises(ValueError):
        bot_actions_reference('hunter', obs[..., :D - 1], rc)
    with pytest.raises(ValueError):
        bot_actions_reference(7, obs, rc)
