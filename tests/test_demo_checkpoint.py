"""The demo CLI's checkpoint options (--checkpoint / --opponent / --greedy):
parsing and refusals on the CPU; a greedy one-env episode with a GIF and a
batched match on the GPU, from a bare {'policy': state_dict} file."""
import pytest

from masurvival import demo


def test_parser_defaults_keep_the_random_policy():
    a = demo.build_parser().parse_args([])
    assert (a.policy, a.checkpoint, a.opponent, a.greedy) == ('random', None, None, False)
    a = demo.build_parser().parse_args(['--checkpoint', 'a.pt', '--opponent', 'b.pt', '--greedy'])
    assert (a.policy, a.checkpoint, a.opponent, a.greedy) == ('random', 'a.pt', 'b.pt', True)
    demo.check_supported(a)


@pytest.mark.parametrize('argv', [['--opponent', 'b.pt'], ['--greedy'], ['--envs', '4', '--greedy']])
def test_opponent_or_greedy_without_checkpoint_exits(argv):
    with pytest.raises(SystemExit, match='--checkpoint'):
        demo.main(argv)


def _bare_checkpoint(tmp_path, config=None):
    import torch
    from masurvival.ppo import PolicyMLP
    from masurvival.vec_env import VecMaSurvival
    env = VecMaSurvival(config, n_envs=1)
    D = env.obs_dim
    env.close()
    torch.manual_seed(D)
    path = tmp_path / 'bare.pt'
    torch.save({'policy': PolicyMLP(D).state_dict()}, path)
    return str(path)


@pytest.mark.gpu
def test_greedy_checkpoint_episode_writes_a_gif(tmp_path, capsys):
    p = _bare_checkpoint(tmp_path)
    gif = tmp_path / 'out.gif'
    assert demo.main(['--checkpoint', p, '--greedy', '--max-steps', '12', '-g', str(gif)]) == 0
    assert gif.stat().st_size > 0
    assert 'Episode complete' in capsys.readouterr().out


@pytest.mark.gpu
def test_batched_match_of_two_checkpoints_prints_wins(tmp_path, capsys):
    p = _bare_checkpoint(tmp_path)
    assert demo.main(['--envs', '64', '--checkpoint', p, '--opponent', p, '--max-steps', '20']) == 0
    out = capsys.readouterr().out
    assert "'wins'" in out and "'episodes'" in out
