"""Play saved policies against each other in one batched env.

``load_policy`` reads the ``'policy'`` entry of a checkpoint (what
``PPOTrainer.save`` writes, or a bare ``{'policy': state_dict}`` file) into a
``PolicyMLP``.  ``Match`` steps an auto-resetting ``VecMaSurvival`` in which
every agent is driven by one of up to two policies, and keeps the score on the
device: per finished episode, which side's summed return was larger.

On a GPU each policy is packed once into a ``FusedPolicy`` and acts only on its
own agents' rows through ``mas_policy_act_sel`` (include/masurvival.h): the
policies' masks are disjoint, so they fill disjoint rows of one actions buffer
and share the RNG key ``(seed, t)``.  On the CPU (a scripted env double) the
torch fp32 forward and ``sample_actions`` stand in.

Either side may be a scripted bot (``masurvival.bots``: a ``Bot`` or a
``'bot:NAME'`` string) instead of a policy: a fixed yardstick that does not
move between runs.  On a GPU its rows are filled by ``mas_bot_act`` with the
mask ``act_sel`` would get, on the CPU by ``bot_actions_reference``; a bot draws
no random numbers, and the policies' rows and RNG keys are what they are
without it.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from .bots import Bot, bot_act, bot_actions_reference, is_bot_spec, parse_bot
from .ppo import HEADS, FusedPolicy, ObsNorm, PolicyMLP, sample_actions

_COUNT_EVERY = 32  # run(episodes=...) reads the device's episode count every this many steps


def load_policy(src, device='cpu') -> PolicyMLP:
    """The PolicyMLP of a checkpoint: `src` is a path (read with
    ``weights_only=True``) or an already loaded dict; only ``src['policy']`` is
    read, and obs_dim comes from ``body.0.weight``.  A checkpoint with an
    ``'obs_norm'`` entry (``PPOConfig.obs_norm``) gives a policy with that
    normaliser attached: it acts on raw observations as the trainer's did."""
    if isinstance(src, (str, bytes, os.PathLike)):
        src = torch.load(src, map_location='cpu', weights_only=True)
    sd = src['policy']
    hidden, obs_dim = sd['body.0.weight'].shape
    policy = PolicyMLP(int(obs_dim), int(hidden))
    policy.load_state_dict(sd)
    if 'obs_norm' in src:
        on = ObsNorm.from_state_dict(src['obs_norm'], 'cpu')
        policy.set_obs_norm(on.mean, on.inv_std)
    return policy.to(device).eval()


def resolve_player(p, device='cpu'):
    """One entry of a `policies` list as Match takes them: a PolicyMLP (as it
    is), a bot (a Bot or a 'bot:NAME' string -> Bot), or a checkpoint (a path
    or a loaded dict -> load_policy)."""
    if isinstance(p, (PolicyMLP, Bot)):
        return p
    if is_bot_spec(p):
        return parse_bot(p)
    if isinstance(p, (str, bytes, os.PathLike, dict)):
        return load_policy(p, device)
    return p


def greedy_actions(raw):
    """Per-head arg-max (the first index wins a tie) of raw [.., 16] head
    outputs; int8 [.., 6]."""
    acts, off = [], 0
    for n in HEADS:
        acts.append(torch.argmax(raw[..., off:off + n], dim=-1))
        off += n
    return torch.stack(acts, dim=-1).to(torch.int8)


def _mask_of(sides: Sequence[int], side: int) -> int:
    return sum(1 << a for a, s in enumerate(sides) if s == side)


class Actor:
    """Actions for [n_envs, n_agents] rows from one or two policies.

    `assignment[a]` is the policy index of agent a; with `swap_sides` the envs
    [n_envs // 2, n_envs) use the inverted assignment.  ``act(src, t, out)``
    fills out int8 [n_envs, n_agents, 6]: on a GPU `src` is the bf16 row buffer
    [n_envs * n_agents, Dx] (``x_buffer``), on the CPU the fp32 obs
    [n_envs, n_agents, obs_dim].

    A side may be a bot (a Bot or 'bot:NAME'); then `config` (the env's
    ResolvedConfig, or its mas_config struct) is needed: the rule reads the
    row's layout and its thresholds from it."""

    def __init__(self, policies, n_envs, n_agents, obs_dim, device, assignment=None, greedy=False, seed=0,
                 swap_sides=False, config=None):
        policies = [resolve_player(p, device) for p in policies]
        if len(policies) not in (1, 2):
            raise ValueError(f'need one or two policies, got {len(policies)}')
        self.cfg_struct = None
        if any(isinstance(p, Bot) for p in policies):
            if config is None:
                raise ValueError('a bot needs the env config (config=, or an env with .rc)')
            self.cfg_struct = config.to_struct() if hasattr(config, 'to_struct') else config
            if int(self.cfg_struct.n_agents) != int(n_agents):
                raise ValueError(f'config n_agents {int(self.cfg_struct.n_agents)} does not match n_agents {n_agents}')
        for p in policies:
            if isinstance(p, Bot):
                continue
            d = p.body[0].weight.shape[1]
            if d != obs_dim:
                raise ValueError(f'policy obs_dim {d} does not match the env obs_dim {obs_dim}')
        self.N, self.A, self.D = int(n_envs), int(n_agents), int(obs_dim)
        if not 1 <= self.A <= 32:
            raise ValueError(f'n_agents {self.A} outside 1..32')
        self.device = torch.device(device)
        if assignment is None:
            assignment = [0] * self.A if len(policies) == 1 else [int(a >= self.A // 2) for a in range(self.A)]
        assignment = [int(a) for a in assignment]
        if len(assignment) != self.A or any(a not in (0, 1) for a in assignment):
            raise ValueError(f'assignment must be {self.A} policy indices in (0, 1)')
        if len(policies) == 1 and any(assignment) and not swap_sides:
            raise ValueError('assignment names policy 1 but one policy was given')
        if swap_sides and self.N % 2 != 0:
            raise ValueError(f'swap_sides needs an even n_envs, got {self.N}')
        self.greedy, self.seed = bool(greedy), int(seed)
        # env slices [lo, hi) with their side per agent; side s is played by
        # policies[s] (by the one policy when only one was given)
        inv = [1 - a for a in assignment]
        self.slices = ([(0, self.N // 2, assignment), (self.N // 2, self.N, inv)] if swap_sides
                       else [(0, self.N, assignment)])
        self.side = torch.zeros((self.N, self.A), dtype=torch.bool, device=self.device)  # True: side 1
        for lo, hi, sides in self.slices:
            self.side[lo:hi] = torch.tensor(sides, dtype=torch.bool, device=self.device)
        self.policies = [policies[min(s, len(policies) - 1)] for s in (0, 1)]
        self.fused = None
        if self.device.type == 'cuda':
            fps = [None if isinstance(p, Bot) else FusedPolicy(p, self.D, self.device) for p in policies]
            for fp in fps:
                if fp is not None:
                    fp.pack()
            self.fused = [fps[min(s, len(fps) - 1)] for s in (0, 1)]
            M = self.N * self.A
            self.logp = torch.empty((M,), dtype=torch.float32, device=self.device)
            self.value = torch.empty((M,), dtype=torch.float32, device=self.device)
        else:
            self.gen = torch.Generator(device='cpu')
            self.gen.manual_seed(self.seed)

    def x_buffer(self):
        """bf16 rows [n_envs * n_agents, Dx] as FusedPolicy.x_buffer lays them
        out (the bias column at index D = 1); made here, since a side may be a
        bot and have no FusedPolicy."""
        Dx = 16 * ((self.D + 1 + 15) // 16)
        x = torch.zeros((self.N * self.A, Dx), dtype=torch.bfloat16, device=self.device)
        x[..., self.D] = 1.0
        return x

    @torch.no_grad()
    def act(self, src, t, out):
        A = self.A
        if self.fused is not None:
            acts = out.view(self.N * A, 6)
            for lo, hi, sides in self.slices:
                r0, r1 = lo * A, hi * A
                for s in (0, 1):
                    mask = _mask_of(sides, s)
                    if mask == 0 or r1 == r0:
                        continue  # this side has no agent in the slice: its policy is not called
                    if isinstance(self.policies[s], Bot):
                        bot_act(self.cfg_struct, self.policies[s], src[r0:r1], A, mask, acts[r0:r1])
                        continue
                    self.fused[s].act_sel(src[r0:r1], A, mask, self.seed, t, acts[r0:r1], self.logp[r0:r1],
                                          self.value[r0:r1], greedy=self.greedy, first_row=r0)
            return out
        for s in (0, 1):
            sel = self.side if s == 1 else ~self.side
            if not bool(sel.any()):
                continue
            if isinstance(self.policies[s], Bot):
                a = bot_actions_reference(self.policies[s], src, self.cfg_struct).to(out.device)
                out.copy_(torch.where(sel.unsqueeze(-1), a, out))
                continue
            raw = self.policies[s].forward_raw(src.float())
            a = greedy_actions(raw) if self.greedy else sample_actions(raw[..., :sum(HEADS)], self.gen)[0]
            out.copy_(torch.where(sel.unsqueeze(-1), a, out))
        return out


class Match:
    """One or two policies in `env` (a VecMaSurvival, or anything with its
    reset / step / n_envs / n_agents / obs_dim / device / auto_reset surface).
    Each may be a PolicyMLP, a checkpoint (path or loaded dict) or a bot (a Bot
    or 'bot:NAME'; the env then needs its ResolvedConfig as `.rc`).

    The act RNG key is (seed, t), t counting this match's steps from 0.
    ``step()`` advances every env one step and returns (rewards [N, A], dones
    [N]); ``run()`` returns ``result()``, a dict of plain numbers.  An episode
    is scored when its env reports done: the two sides' returns summed over
    their agents are compared under that env's assignment."""

    def __init__(self, env, policies, assignment: Optional[Sequence[int]] = None, greedy: bool = False,
                 seed: int = 0, swap_sides: bool = False):
        if not getattr(env, 'auto_reset', False):
            raise ValueError('Match needs an auto-resetting env (auto_reset=True)')
        policies = [resolve_player(p, env.device) for p in policies]
        dims = [int(p.body[0].weight.shape[1]) for p in policies if not isinstance(p, Bot)]
        if any(d != env.obs_dim for d in dims):
            raise ValueError(f'policy obs_dim {dims} does not match the env obs_dim {env.obs_dim}')
        self.env = env
        N, A = int(env.n_envs), int(env.n_agents)
        dev = torch.device(env.device)
        self.actor = Actor(policies, N, A, env.obs_dim, dev, assignment, greedy, seed, swap_sides,
                           config=getattr(env, 'rc', None))
        self.on_gpu = dev.type == 'cuda'
        self.use_step_x = bool(self.on_gpu and hasattr(env, 'step_x') and env.supports_step_x())
        self.actions = torch.zeros((N, A, 6), dtype=torch.int8, device=dev)
        self.x = self.actor.x_buffer() if self.on_gpu else None
        if self.use_step_x:
            self.rewards = torch.zeros((N, A), dtype=torch.float32, device=dev)
            self.dones = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self.side1 = self.actor.side.to(torch.float64)
        self.reset()

    def _take_obs(self, obs):
        if self.on_gpu:
            D = self.env.obs_dim
            self.x[:, :D].copy_(obs.reshape(-1, D))  # fp32 -> bf16, round to nearest even
        else:
            self.obs = obs

    def reset(self):
        """Reset every env, the step counter and the score."""
        N, A, dev = self.actor.N, self.actor.A, self.actor.device
        self.t = 0
        self._ret = torch.zeros((N, A), dtype=torch.float64, device=dev)  # running per-agent return
        self._len = torch.zeros((N,), dtype=torch.int64, device=dev)
        self._wins = torch.zeros((2,), dtype=torch.int64, device=dev)
        self._draws = torch.zeros((), dtype=torch.int64, device=dev)
        self._episodes = torch.zeros((), dtype=torch.int64, device=dev)
        self._ret_sum = torch.zeros((2,), dtype=torch.float64, device=dev)
        self._len_sum = torch.zeros((), dtype=torch.int64, device=dev)
        self._take_obs(self.env.reset())

    @torch.no_grad()
    def step(self):
        self.actor.act(self.x if self.on_gpu else self.obs, self.t, self.actions)
        if self.use_step_x:
            self.env.step_x(self.actions, self.x, self.rewards, self.dones)
            rewards, dones = self.rewards, self.dones
        else:
            obs, rewards, dones = self.env.step(self.actions)[:3]
            self._take_obs(obs)
        self.t += 1
        self._account(rewards, dones)
        return rewards, dones

    def _account(self, rewards, dones):
        d = dones.to(torch.bool)
        self._ret += rewards
        self._len += 1
        s1 = (self._ret * self.side1).sum(1)
        s0 = (self._ret * (1.0 - self.side1)).sum(1)
        self._wins[0] += (d & (s0 > s1)).sum()
        self._wins[1] += (d & (s1 > s0)).sum()
        self._draws += (d & (s0 == s1)).sum()
        self._episodes += d.sum()
        self._ret_sum[0] += torch.where(d, s0, torch.zeros_like(s0)).sum()
        self._ret_sum[1] += torch.where(d, s1, torch.zeros_like(s1)).sum()
        self._len_sum += torch.where(d, self._len, torch.zeros_like(self._len)).sum()
        self._ret.masked_fill_(d.unsqueeze(1), 0.0)
        self._len.masked_fill_(d, 0)

    def result(self):
        """Finished episodes only: episodes, steps (of this match), wins per
        side, draws, each side's mean per-episode return, mean episode length."""
        n = int(self._episodes.item())
        wins = [int(w) for w in self._wins.tolist()]
        rs = self._ret_sum.tolist()
        return {'episodes': n, 'steps': self.t, 'wins': wins, 'draws': int(self._draws.item()),
                'return': [float(r) / n if n else 0.0 for r in rs],
                'mean_length': float(self._len_sum.item()) / n if n else 0.0}

    def run(self, steps: Optional[int] = None, episodes: Optional[int] = None, max_steps: Optional[int] = None):
        """`steps` steps, or until at least `episodes` episodes have finished
        (the count is read every 32 steps) or `max_steps` steps have run."""
        if (steps is None) == (episodes is None):
            raise ValueError('give either steps or episodes')
        if steps is not None:
            for _ in range(int(steps)):
                self.step()
            return self.result()
        if max_steps is None:
            raise ValueError('episodes mode needs max_steps')
        done = 0
        while done < int(max_steps):
            self.step()
            done += 1
            if done % _COUNT_EVERY == 0 and int(self._episodes.item()) >= int(episodes):
                break
        return self.result()
