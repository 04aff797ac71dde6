"""On-device PPO rollout for VecMaSurvival.

The reference ships no trainer; this is the consumer the batched env step is
built for.  Everything stays in HBM:

* ``RolloutBuffer`` -- obs [T+1, N, A, D] (the env kernel writes each step's
  observation straight into row t+1), actions int8 [T, N, A, 6], log-probs,
  values [T+1, N, A], rewards [T, N, A], dones uint8 [T, N]; advantages and
  returns [T, N, A].
* GAE(gamma, lambda) is the HIP ``mas_gae`` kernel (one lane per agent
  column, backward over T), which also returns the fp64 advantage sums.
* The policy is a shared-parameter MLP (obs D -> 256 -> 256, tanh) with six
  categorical heads (MultiDiscrete [3,3,3,2,2,2]) and a value head; forward
  passes run under bf16 autocast (hipBLASLt GEMMs), losses in fp32.

Multi-GPU (one process per GPU, envs sharded): the only collectives are one
fp64 all-reduce of (sum adv, sum adv^2, count) per rollout and one flat
gradient all-reduce (average) per minibatch -- RCCL over xGMI when the process
group is 'nccl', gloo in the CPU tests.

Self-play (``PPOTrainer(opponent=..., learner_agents=...)``): a frozen opponent
drives the agents the trained policy does not own.  Both act in one rollout
(two ``mas_policy_act_sel`` calls per step into one actions buffer); after it
the learner's rows are gathered once into dense buffers (``mas_rows_select``,
``RolloutBuffer.learner``), and GAE, the advantage statistics and the update
run on those alone.

Dead agents (``PPOConfig.mask_dead``): the env ignores a dead agent's actions
until the episode ends, so its rows carry no policy signal.  With the flag on,
``RolloutBuffer.active`` records ``env.alive()`` before every step, the
advantages are normalised over the active rows, and each minibatch weights a
row's surrogate and entropy terms by ``active * rows / sum(active)`` (zeros
where a minibatch has no active row): ``pg``, ``entropy`` and ``clipfrac`` become
means over the active rows.  The value loss stays a mean over all rows: a dead
agent keeps receiving reward, and a live row's GAE bootstraps from the value of
the next, possibly dead, row.  Multi-GPU: every rank normalises its minibatch by
its own active count and the ranks' gradients are averaged as before, so a rank
with few active rows weighs each of them more than a global normalisation
would -- an approximation that costs no extra collective.

Observation normalisation (``PPOConfig.obs_norm``): a running per-column mean
and variance of the policy's bf16 input rows (``ObsNorm``: ``mas_obs_stats``
over the rollout's rows, Chan's merge in fp64), folded into the packed layer-1
weights (``mas_policy_pack_norm``) instead of applied to a row: the act and
train kernels and the rollout buffer keep raw rows.  The constructor merges the
reset rows, ``iteration()`` merges the rows it has just trained on and packs
again, so rollout k and update k see one normaliser (the reset rows are
counted twice, once in a lifetime: as block 0 of the first rollout too).
Nothing clips a normalised value: ``obs_norm_eps`` (the variance floor) is the
only bound, ``inv_std <= 1 / sqrt(eps)`` (10 by default).

Reward normalisation (``PPOConfig.reward_norm``): VecNormalize's other half.
Every agent column keeps a running discounted return R across rollouts
(``RetNorm.carry``); after a rollout (and the learner's row selection)
``mas_ret_stats`` walks it forward and sums R and R^2 in fp64, the record is
all-reduced and merged (Chan, ``mas_obs_norm_merge`` with one column), and GAE
(``mas_gae_scaled``) reads ``clamp(r * scale, -reward_clip, reward_clip)`` with
``scale = 1 / sqrt(var(R) + reward_norm_eps)`` from device memory.  The rollout's
own returns are merged before its rewards are scaled; the mean is not
subtracted; the rewards buffer keeps the raw rewards.

Episode statistics (``PPOConfig.episode_stats``): what the rollouts' own
episodes looked like.  After a rollout, before the learner's row selection,
``mas_episode_stats`` walks the whole buffer's rewards and dones forward, one
thread per env, from per-env carries of every agent's undiscounted return and
of the episode length (``EpisodeStats``), and leaves one fp64 record: episodes
finished, sums of their lengths and of every agent slot's return (and of the
squares), wins per side and draws by Match's rule.  The record is all-reduced,
added to a lifetime total, and ``last_stats`` gains ``episodes``,
``ep_length``, ``ep_return`` and ``win_rate`` as device tensors;
``episode_summary()`` is the only host copy.  Side 0 is the learner's agents
when there is an opponent, otherwise agents ``range(A // 2)``.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from .abi import MAS_ERR_UNSUPPORTED, MasError, check, load_library

HEADS = (3, 3, 3, 2, 2, 2)
N_LOGITS = sum(HEADS)

# MAS_ROCTX=1 brackets the trainer's phases (rollout, gae, update) with roctx
# ranges (torch.cuda.nvtx is roctx on ROCm) for rocprofv3 --marker-trace.
_ROCTX = os.environ.get('MAS_ROCTX', '0') == '1'


class _phase:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _ROCTX:
            torch.cuda.nvtx.range_push(self.name)

    def __exit__(self, *exc):
        if _ROCTX:
            torch.cuda.nvtx.range_pop()


@dataclass
class PPOConfig:
    horizon: int = 64          # T
    gamma: float = 0.99
    lam: float = 0.95
    hidden: int = 256
    lr: float = 3e-4
    epochs: int = 1
    minibatches: int = 4
    clip: float = 0.2
    vf_coef: float = 0.5
    ent_coef: float = 0.01
    max_grad_norm: float = 0.5
    autocast_bf16: bool = True
    # fused HIP policy kernels (mas_policy_act / mas_policy_train): default on
    # a GPU when hidden == 256; the torch path stays as the CPU / reference path
    fused: Optional[bool] = None
    # the advantage-statistics and gradient all-reduces: None = when the
    # process group has more than one rank; True forces them at world size 1
    # too (the one-GPU RCCL test runs the exact calls of the 8-GPU bench)
    allreduce: Optional[bool] = None
    # fused path: the env writes the policy's bf16 input rows itself
    # (mas_step_x) instead of fp32 obs rows the act kernel re-reads and
    # converts; None = whenever the env supports it (same bits either way)
    x_obs: Optional[bool] = None
    # self-play (PPOTrainer(opponent=...)): copy the learner's weights into the
    # opponent after every k-th iteration() (lagged self-play); 0 = never
    opponent_sync_every: int = 0
    # weight the policy terms of the loss (surrogate, entropy) by the agents'
    # alive flags (env.alive()), see the module docstring; off: every row alike
    mask_dead: bool = False
    # running per-column mean / variance normalisation of the observations,
    # folded into the packed layer-1 weights (module docstring); off: the same
    # launches and bits as without it
    obs_norm: bool = False
    # the variance floor: inv_std = 1 / sqrt(var + eps) <= 1 / sqrt(eps).  The
    # fold cannot clip a normalised value (VecNormalize clips at +-10), so
    # this alone bounds how far a near-constant column is amplified
    obs_norm_eps: float = 1e-2
    # running return normalisation of the rewards (module docstring): GAE reads
    # clamp(r / sqrt(var(R) + reward_norm_eps), -reward_clip, reward_clip), R the
    # columns' running discounted returns; off: the same launches and bits as
    # without it
    reward_norm: bool = False
    reward_norm_eps: float = 1e-8
    reward_clip: float = 10.0
    # episode statistics of the training rollouts (module docstring): returns,
    # lengths and wins of the episodes each rollout finished, kept on the
    # device; it only reads the buffer.  Off: the same launches and bits as
    # without it
    episode_stats: bool = False


def _split_k(m: int, cap: int = int(os.environ.get('MAS_SPLITK_CAP', '128'))) -> int:
    c = 1
    while c < cap and m % (2 * c) == 0 and m // (2 * c) >= 4096:
        c *= 2
    return c


class _LinearSplitKFn(torch.autograd.Function):
    """y = x W^T + b whose weight gradient is computed split-K: for a PPO
    minibatch of millions of rows, dW = dY^T X has a tiny M x N and a huge K,
    and a single GEMM there launches a handful of tiles; a batched GEMM over
    row chunks followed by a sum fills the GPU."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        x2 = x.reshape(-1, x.shape[-1])
        g2 = gy.reshape(-1, gy.shape[-1])
        gx = (g2 @ w).reshape(x.shape) if ctx.needs_input_grad[0] else None
        m = x2.shape[0]
        c = _split_k(m)
        gw = torch.bmm(g2.reshape(c, m // c, -1).transpose(1, 2), x2.reshape(c, m // c, -1)).sum(0)
        gb = g2.reshape(c, m // c, -1).sum(1).sum(0)
        return gx, gw.to(w.dtype), gb


class LinearSplitK(nn.Linear):
    def forward(self, x):
        if torch.is_autocast_enabled(x.device.type):
            dt = torch.get_autocast_dtype(x.device.type)
            with torch.autocast(x.device.type, enabled=False):
                return _LinearSplitKFn.apply(x.to(dt), self.weight.to(dt), self.bias.to(dt))
        return _LinearSplitKFn.apply(x, self.weight, self.bias)


class PolicyMLP(nn.Module):
    """Shared across agents: obs [.., D] -> (logits [.., 15], value [..])."""

    def __init__(self, obs_dim: int, hidden: int = 256):
        super().__init__()
        self.body = nn.Sequential(LinearSplitK(obs_dim, hidden), nn.Tanh(), LinearSplitK(hidden, hidden), nn.Tanh())
        self.head = LinearSplitK(hidden, N_LOGITS + 1)
        # the optional input normaliser (set_obs_norm): non-persistent buffers,
        # so state_dict() keeps its keys and old checkpoints load, while
        # deepcopy and .to() carry them along
        self.register_buffer('obs_mean', None, persistent=False)
        self.register_buffer('obs_inv_std', None, persistent=False)

    def set_obs_norm(self, mean, inv_std):
        """Attach (mean, inv_std) [obs_dim] -- the tensors themselves, so an
        ObsNorm that updates them in place updates this policy -- or detach
        with (None, None): forward then computes on (x - mean) * inv_std."""
        if (mean is None) != (inv_std is None):
            raise ValueError('set_obs_norm: mean and inv_std go together')
        if mean is not None:
            d = self.body[0].weight.shape[1]
            if mean.shape != (d,) or inv_std.shape != (d,):
                raise ValueError(f'set_obs_norm: expected two [{d}] tensors, got {tuple(mean.shape)} and '
                                 f'{tuple(inv_std.shape)}')
        self.obs_mean, self.obs_inv_std = mean, inv_std

    def _normed(self, x):
        if self.obs_mean is None:
            return x
        return (x - self.obs_mean) * self.obs_inv_std

    def forward(self, x):
        h = self.head(self.body(self._normed(x)))
        return h[..., :N_LOGITS].float(), h[..., N_LOGITS].float()

    def forward_raw(self, x):
        """[.., 16] fp32 head output: 15 logits then the value."""
        return self.head(self.body(self._normed(x))).float()


def _split_heads(logits):
    return torch.split(logits, HEADS, dim=-1)


def sample_actions(logits, gen: Optional[torch.Generator] = None):
    """Gumbel-max sample of the six heads; returns (int8 [.., 6], logp [..])."""
    acts, logp = [], 0.0
    for lg in _split_heads(logits):
        lsm = F.log_softmax(lg, dim=-1)
        u = torch.rand(lg.shape, device=lg.device, generator=gen).clamp_(1e-20, 1.0)
        a = torch.argmax(lsm - torch.log(-torch.log(u)), dim=-1)
        acts.append(a)
        logp = logp + lsm.gather(-1, a.unsqueeze(-1)).squeeze(-1)
    return torch.stack(acts, dim=-1).to(torch.int8), logp


def sample_actions_hip(logits, seed, step, actions_out, logp_out):
    """HIP sampler (include/masurvival.h mas_sample_actions): logits [M, >=15]
    fp32 with unit column stride; writes actions_out int8 [M, 6], logp_out [M]."""
    lib = load_library()
    M = logits.shape[0]
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.stride(1) == 1
    assert actions_out.is_contiguous() and logp_out.is_contiguous()
    check(lib.mas_sample_actions(M, ctypes.c_void_p(logits.data_ptr()), logits.stride(0), seed, step,
                                 ctypes.c_void_p(actions_out.data_ptr()), ctypes.c_void_p(logp_out.data_ptr()),
                                 ctypes.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)))


def evaluate_actions(logits, actions):
    """log-prob and entropy of given actions [.., 6]."""
    logp, ent = 0.0, 0.0
    a = actions.long()
    for k, lg in enumerate(_split_heads(logits)):
        lsm = F.log_softmax(lg, dim=-1)
        logp = logp + lsm.gather(-1, a[..., k:k + 1]).squeeze(-1)
        ent = ent - (lsm.exp() * lsm).sum(-1)
    return logp, ent


def gae_scratch(n_columns, device):
    """The partial-sum scratch one mas_gae call needs (mas_gae_scratch_doubles)."""
    n = load_library().mas_gae_scratch_doubles(int(n_columns))
    return torch.empty((n,), device=device, dtype=torch.float64)


def gae(rewards, values, dones, gamma, lam, adv_out, ret_out, sums_out, n_agents, stream=None, scratch=None):
    """HIP GAE over [T, N*A] columns (include/masurvival.h mas_gae).  scratch:
    float64 device tensor of mas_gae_scratch_doubles(N*A) (allocated here when
    None); concurrent calls need their own scratch and outputs."""
    lib = load_library()
    T = rewards.shape[0]
    M = rewards[0].numel()
    for t in (rewards, values, adv_out, ret_out):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert values.shape[0] == T + 1 and dones.shape[0] == T and dones.dtype == torch.uint8
    assert dones[0].numel() * n_agents == M and sums_out.dtype == torch.float64
    if scratch is None:
        scratch = gae_scratch(M, rewards.device)
    assert scratch.is_cuda and scratch.dtype == torch.float64 and scratch.numel() >= lib.mas_gae_scratch_doubles(M)
    s = stream if stream is not None else torch.cuda.current_stream(rewards.device).cuda_stream
    check(lib.mas_gae(T, M, n_agents, ctypes.c_void_p(rewards.data_ptr()), ctypes.c_void_p(values.data_ptr()),
                      ctypes.c_void_p(dones.data_ptr()), float(gamma), float(lam),
                      ctypes.c_void_p(adv_out.data_ptr()), ctypes.c_void_p(ret_out.data_ptr()),
                      ctypes.c_void_p(sums_out.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                      ctypes.c_void_p(s)))


def adv_normalize(adv, stats, stream=None):
    """adv (DEVICE fp32, contiguous) normalised in place from stats = fp64
    [sum, sum of squares, count] (include/masurvival.h mas_adv_normalize):
    adv.sub_(mean.float()).div_(var.sqrt().float() + 1e-8), one launch."""
    assert adv.is_cuda and adv.dtype == torch.float32 and adv.is_contiguous()
    assert stats.dtype == torch.float64 and stats.numel() == 3 and stats.is_contiguous()
    lib = load_library()
    st = stream if stream is not None else torch.cuda.current_stream(adv.device).cuda_stream
    check(lib.mas_adv_normalize(adv.numel(), ctypes.c_void_p(adv.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                                ctypes.c_void_p(st)))


def _rollout_columns(name, rewards, dones, n_agents):
    """(T, M) of a [T, ..] fp32 rewards tensor and its [T, envs] uint8 dones on one GPU, or ValueError."""
    if not (isinstance(rewards, torch.Tensor) and rewards.is_cuda and rewards.dtype == torch.float32
            and rewards.dim() >= 2 and rewards.is_contiguous()):
        raise ValueError(f'{name}: rewards must be a contiguous fp32 [T, columns] tensor on a GPU')
    T, M = rewards.shape[0], rewards[0].numel()
    if not (isinstance(dones, torch.Tensor) and dones.device == rewards.device and dones.dtype == torch.uint8
            and dones.is_contiguous() and dones.dim() >= 1 and dones.shape[0] == T
            and dones[0].numel() * int(n_agents) == M):
        raise ValueError(f'{name}: dones must be a contiguous uint8 [T, columns / n_agents] tensor beside the rewards')
    return T, M


def ret_stats(rewards, dones, gamma, carry, sums_out, n_agents, stream=None, scratch=None):
    """HIP running-return statistics over [T, N*A] columns (include/masurvival.h
    mas_ret_stats): carry (fp32 [N*A], each column's discounted return so far)
    is advanced in place through the rollout and sums_out (fp64 [2]) receives
    the sum of the T * N*A returns and of their squares.  scratch: float64
    device tensor of mas_ret_stats_scratch_doubles(N*A) (a gae_scratch is large
    enough; allocated here when None)."""
    lib = load_library()
    if not hasattr(lib, 'mas_ret_stats'):
        raise MasError('the loaded library has no mas_ret_stats')
    T, M = _rollout_columns('ret_stats', rewards, dones, n_agents)
    dev = rewards.device
    if not (carry.device == dev and carry.dtype == torch.float32 and carry.is_contiguous() and carry.numel() == M):
        raise ValueError(f'ret_stats: carry must be a contiguous fp32 tensor of {M} columns on {dev}')
    if not (sums_out.device == dev and sums_out.dtype == torch.float64 and sums_out.is_contiguous()
            and sums_out.numel() == 2):
        raise ValueError('ret_stats: sums_out must be a contiguous fp64 [2] tensor beside the rewards')
    need = int(lib.mas_ret_stats_scratch_doubles(M))
    if scratch is None:
        scratch = torch.empty((need,), device=dev, dtype=torch.float64)
    if not (scratch.device == dev and scratch.dtype == torch.float64 and scratch.numel() >= need):
        raise ValueError(f'ret_stats: scratch must hold {need} fp64 values on {dev}')
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    check(lib.mas_ret_stats(T, M, int(n_agents), ctypes.c_void_p(rewards.data_ptr()),
                            ctypes.c_void_p(dones.data_ptr()), float(gamma), ctypes.c_void_p(carry.data_ptr()),
                            ctypes.c_void_p(sums_out.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                            ctypes.c_void_p(s)))


def gae_scaled(rewards, values, dones, gamma, lam, scale, clip, adv_out, ret_out, sums_out, n_agents, stream=None,
               scratch=None):
    """gae() on clamp(rewards * scale, -clip, clip) without writing the rewards
    (include/masurvival.h mas_gae_scaled).  scale: fp32 [1] DEVICE tensor, read
    by the kernel (no host copy); clip: a positive float, inf for none."""
    lib = load_library()
    if not hasattr(lib, 'mas_gae_scaled'):
        raise MasError('the loaded library has no mas_gae_scaled')
    T = rewards.shape[0]
    M = rewards[0].numel()
    for t in (rewards, values, adv_out, ret_out):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert values.shape[0] == T + 1 and dones.shape[0] == T and dones.dtype == torch.uint8
    assert dones[0].numel() * n_agents == M and sums_out.dtype == torch.float64
    assert scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1
    if scratch is None:
        scratch = gae_scratch(M, rewards.device)
    assert scratch.is_cuda and scratch.dtype == torch.float64 and scratch.numel() >= lib.mas_gae_scratch_doubles(M)
    s = stream if stream is not None else torch.cuda.current_stream(rewards.device).cuda_stream
    check(lib.mas_gae_scaled(T, M, n_agents, ctypes.c_void_p(rewards.data_ptr()), ctypes.c_void_p(values.data_ptr()),
                             ctypes.c_void_p(dones.data_ptr()), float(gamma), float(lam),
                             ctypes.c_void_p(scale.data_ptr()), float(clip),
                             ctypes.c_void_p(adv_out.data_ptr()), ctypes.c_void_p(ret_out.data_ptr()),
                             ctypes.c_void_p(sums_out.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                             ctypes.c_void_p(s)))


def scale_rewards_reference(rewards, scale, clip):
    """Plain torch restatement of mas_gae_scaled's reward: the fp32 product,
    rounded on its own, then the clamp (a NaN passes through)."""
    return torch.clamp(rewards * scale.to(rewards.dtype), -float(clip), float(clip))


def _agent_mask(agents, n_agents, what='agents'):
    """Bit mask of a list of agent indices (unique, in range, non-empty)."""
    agents = [int(a) for a in agents]
    if not agents:
        raise ValueError(f'{what}: no agent given')
    if len(set(agents)) != len(agents):
        raise ValueError(f'{what}: {agents} repeats an agent')
    if min(agents) < 0 or max(agents) >= n_agents:
        raise ValueError(f'{what}: {agents} outside 0..{n_agents - 1}')
    return sum(1 << a for a in agents)


def rows_select(n_agents, agent_mask, x=None, x_out=None, x_cols=None, actions=None, actions_out=None, f32=(),
                stream=None):
    """Gather the rows of the agents bit-selected by agent_mask into dense
    tensors (include/masurvival.h mas_rows_select): every input holds whole
    envs of n_agents rows (row = env * n_agents + agent), every output
    n_envs * popcount(agent_mask) rows in (env, ascending agent) order.
    x / x_out: bf16 [rows, stride] with unit column stride (the row strides
    may differ; columns [0, x_cols) are copied, x_cols defaults to x's
    width); actions / actions_out: int8 [rows, 6]; f32: up to four (in, out)
    pairs of fp32 tensors of rows elements.  Pairs left out are skipped.  One
    launch on the current stream.  A wrong tensor raises ValueError before
    anything reaches the device."""
    n_agents, agent_mask = int(n_agents), int(agent_mask)
    if not 1 <= n_agents <= 32:
        raise ValueError(f'rows_select: n_agents {n_agents} outside 1..32')
    if agent_mask <= 0 or agent_mask >> n_agents:
        raise ValueError(f'rows_select: agent_mask {agent_mask:#x} is zero or has a bit at or above n_agents')
    m = bin(agent_mask).count('1')
    f32 = list(f32)
    if len(f32) > 4:
        raise ValueError(f'rows_select: at most four fp32 pairs, got {len(f32)}')
    if (x is None) != (x_out is None) or (actions is None) != (actions_out is None):
        raise ValueError('rows_select: an input without its output (or the reverse)')
    pairs = []  # (name, in, out, dtype, rows of in, rows of out)
    if x is not None:
        for name, t in (('x', x), ('x_out', x_out)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 != 0:
                raise ValueError(f'rows_select: {name} must be a [rows, stride] tensor with unit column stride and '
                                 'a row stride that is a multiple of 8')
        x_cols = int(x.shape[1] if x_cols is None else x_cols)
        if x_cols <= 0 or x_cols % 8 != 0 or x_cols > x.shape[1] or x_cols > x_out.shape[1]:
            raise ValueError(f'rows_select: x_cols {x_cols} must be a positive multiple of 8 within both widths')
        pairs.append(('x', x, x_out, torch.bfloat16, x.shape[0], x_out.shape[0]))
    if actions is not None:
        for name, t in (('actions', actions), ('actions_out', actions_out)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 6 or not t.is_contiguous():
                raise ValueError(f'rows_select: {name} must be a contiguous [rows, 6] tensor')
        pairs.append(('actions', actions, actions_out, torch.int8, actions.shape[0], actions_out.shape[0]))
    for k, pr in enumerate(f32):
        if len(pr) != 2 or not all(isinstance(t, torch.Tensor) and t.is_contiguous() for t in pr):
            raise ValueError(f'rows_select: f32[{k}] must be an (in, out) pair of contiguous tensors')
        pairs.append((f'f32[{k}]', pr[0], pr[1], torch.float32, pr[0].numel(), pr[1].numel()))
    if not pairs:
        return
    rows = pairs[0][4]
    if rows % n_agents != 0:
        raise ValueError(f'rows_select: {rows} rows are not whole envs of {n_agents} agents')
    n_envs = rows // n_agents
    dev = pairs[0][1].device
    for name, ti, to, dt, ri, ro in pairs:
        if ti.dtype != dt or to.dtype != dt:
            raise ValueError(f'rows_select: {name} must be {dt} (got {ti.dtype} -> {to.dtype})')
        if not (ti.is_cuda and to.is_cuda) or ti.device != dev or to.device != dev:
            raise ValueError(f'rows_select: {name} must live on one GPU (got {ti.device} -> {to.device})')
        if ri != rows or ro != n_envs * m:
            raise ValueError(f'rows_select: {name} has {ri} -> {ro} rows, expected {rows} -> {n_envs * m}')
        if ti.data_ptr() == to.data_ptr() and ri > 0:
            raise ValueError(f'rows_select: {name} is gathered onto itself')
    lib = load_library()
    if not hasattr(lib, 'mas_rows_select'):
        raise MasError('the loaded library has no mas_rows_select')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
    n = len(f32)
    fin = (ctypes.c_void_p * max(n, 1))(*[pr[0].data_ptr() for pr in f32])
    fout = (ctypes.c_void_p * max(n, 1))(*[pr[1].data_ptr() for pr in f32])
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    check(lib.mas_rows_select(n_envs, n_agents, agent_mask, ptr(x), x.stride(0) if x is not None else 0, ptr(x_out),
                              x_out.stride(0) if x is not None else 0, x_cols if x is not None else 0,
                              ptr(actions), ptr(actions_out), n, fin, fout, ctypes.c_void_p(st)))


def obs_moments_reference(x_rows, n_cols):
    """Plain torch restatement of mas_obs_stats: fp64 [2, n_cols], the sums
    and the sums of squares of columns [0, n_cols) over all rows of x_rows
    [.., >= n_cols] (bf16 rows, or anything exactly representable in fp64)."""
    x = x_rows.reshape(-1, x_rows.shape[-1])[:, :n_cols].to(torch.float64)
    return torch.stack([x.sum(0), (x * x).sum(0)])


def merge_reference(state, batch, eps):
    """Plain torch fp64 restatement of mas_obs_norm_merge: state
    [1 + 2 n_cols] = (count, mean, m2) is updated in place from batch
    [1 + 2 n_cols] = (count_b, sums, sums of squares); returns the fp32
    (mean, inv_std), the identity (0, 1) while the count is 0."""
    n_cols = (state.numel() - 1) // 2
    count, nb = state[0].clone(), batch[0]
    mean, m2 = state[1:1 + n_cols], state[1 + n_cols:]
    n = count + nb
    if float(nb) > 0:
        mean_b = batch[1:1 + n_cols] / nb
        m2_b = (batch[1 + n_cols:] - nb * mean_b * mean_b).clamp_min(0.0)
        d = mean_b - mean
        mean += d * nb / n
        m2 += m2_b + d * d * count * nb / n
        state[0] = n
    if float(n) > 0:
        return mean.float(), (1.0 / torch.sqrt(m2 / n + eps)).float()
    return torch.zeros_like(mean, dtype=torch.float32), torch.ones_like(mean, dtype=torch.float32)


def unfold_dw1(g1w, g1b, mean, inv_std):
    """dL/dW1 of the normalised form h = W1 ((x - mean) * inv_std) + b1 from
    the gradient (g1w [F, D], g1b [F]) of the folded form h = W1' x + b1' the
    kernels compute on raw rows (W1' = W1 diag(inv_std), b1' = b1 - W1' mean):
    dW1 = (g1w - g1b (x) mean) * inv_std.  db1 is g1b itself."""
    return (g1w - g1b.unsqueeze(1) * mean) * inv_std


class ObsNorm:
    """Running per-column mean / variance of the policy's input rows: the fp64
    state (count, mean[], m2[]) and the fp32 ``mean`` / ``inv_std`` made from
    it (inv_std = 1 / sqrt(m2 / count + eps); 0 and 1 while the count is 0),
    all on `device`.  On a GPU ``update`` is mas_obs_stats + mas_obs_norm_merge
    (include/masurvival.h); ``update_reference`` and the CPU are the torch
    restatement (obs_moments_reference, merge_reference).  ``mean`` and
    ``inv_std`` are updated in place: a PolicyMLP they are attached to
    (set_obs_norm) follows."""

    def __init__(self, n_cols, device, eps=1e-2):
        self.n_cols, self.device, self.eps = int(n_cols), torch.device(device), float(eps)
        self.state = torch.zeros((1 + 2 * self.n_cols,), dtype=torch.float64, device=self.device)
        self.batch = torch.zeros_like(self.state)
        self.mean = torch.zeros((self.n_cols,), dtype=torch.float32, device=self.device)
        self.inv_std = torch.ones((self.n_cols,), dtype=torch.float32, device=self.device)
        self._scratch = None
        self.lib = None
        if self.device.type == 'cuda':
            self.lib = load_library()
            if not hasattr(self.lib, 'mas_obs_stats'):
                raise MasError('the loaded library has no mas_obs_stats')

    @property
    def count(self):
        return self.state[0]

    def _merge(self, group, reduce):
        if reduce:
            dist.all_reduce(self.batch, group=group)
        if self.lib is not None:
            ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            check(self.lib.mas_obs_norm_merge(self.n_cols, ptr(self.state), ptr(self.batch), self.eps, ptr(self.mean),
                                              ptr(self.inv_std),
                                              ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        else:
            mean, inv_std = merge_reference(self.state, self.batch, self.eps)
            self.mean.copy_(mean)
            self.inv_std.copy_(inv_std)

    @torch.no_grad()
    def update(self, x_rows_bf16, group=None, reduce=None):
        """Merge the bf16 rows x_rows_bf16 [rows, stride] (unit column stride,
        a row stride that is a multiple of 8; columns [0, n_cols) count) into
        the state.  reduce (default: whether a group is given): all-reduce the
        batch record (count, sums, sums of squares) over `group` first, so
        every rank ends with the same state."""
        x = x_rows_bf16
        if x.dtype != torch.bfloat16 or x.dim() != 2 or x.shape[1] < self.n_cols or x.device.type != self.device.type:
            raise ValueError(f'ObsNorm.update: need bf16 [rows, >= {self.n_cols}] rows on {self.device}')
        if self.lib is None:
            return self.update_reference(x, group, reduce)
        self.batch[:1].fill_(float(x.shape[0]))  # (the all-reduce sums the ranks' counts in place)
        if x.stride(1) != 1 or x.stride(0) % 8 != 0:
            raise ValueError('ObsNorm.update: rows need unit column stride and a row stride that is a multiple of 8')
        need = int(self.lib.mas_obs_stats_scratch_doubles(x.shape[0], self.n_cols))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty((max(need, 1),), dtype=torch.float64, device=self.device)
        check(self.lib.mas_obs_stats(x.shape[0], self.n_cols, ctypes.c_void_p(x.data_ptr()), x.stride(0),
                                     ctypes.c_void_p(self.batch.data_ptr() + 8),
                                     ctypes.c_void_p(self._scratch.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._merge(group, group is not None if reduce is None else reduce)

    @torch.no_grad()
    def update_reference(self, x_rows, group=None, reduce=None):
        """update() with the moments from the torch restatement: for rows that
        are not the kernels' (any row stride, any device)."""
        self.batch[:1].fill_(float(x_rows.reshape(-1, x_rows.shape[-1]).shape[0]))
        self.batch[1:].copy_(obs_moments_reference(x_rows, self.n_cols).reshape(-1))
        self._merge(group, group is not None if reduce is None else reduce)

    @torch.no_grad()
    def refresh(self):
        """mean / inv_std again from the state (a merge of an empty batch)."""
        self.batch.zero_()
        self._merge(None, False)

    def state_dict(self):
        n = self.n_cols
        return {'count': self.state[0].detach().clone(), 'mean': self.state[1:1 + n].detach().clone(),
                'm2': self.state[1 + n:].detach().clone(), 'eps': float(self.eps)}

    @torch.no_grad()
    def load_state_dict(self, sd):
        n = self.n_cols
        if sd['mean'].shape != (n,) or sd['m2'].shape != (n,):
            raise ValueError(f'ObsNorm: checkpoint statistics of {tuple(sd["mean"].shape)} columns, expected {n}')
        self.state[0] = sd['count'].to(torch.float64)
        self.state[1:1 + n].copy_(sd['mean'])
        self.state[1 + n:].copy_(sd['m2'])
        self.eps = float(sd.get('eps', self.eps))
        self.refresh()

    @classmethod
    def from_state_dict(cls, sd, device):
        on = cls(sd['mean'].numel(), device, sd.get('eps', 1e-2))
        on.load_state_dict(sd)
        return on


def ret_stats_reference(rewards, dones, gamma, carry, n_agents, steps_out=None):
    """Plain torch restatement of mas_ret_stats in fp32 (the CPU trainer's;
    tests/ret_ref.py holds it to fp64): returns (the new carry [columns], the
    fp64 sums [2] of the T * columns running returns and of their squares).
    Per step R = fl32(fl32(gamma * R) + r) (two torch ops, so two roundings),
    R and R^2 counted in double, then R = 0 where the column's env is done (any
    nonzero byte).  `carry` is not written.  steps_out: an optional [T, columns]
    tensor that receives every step's R as it was counted."""
    T = rewards.shape[0]
    r = rewards.reshape(T, -1)
    d = (dones.reshape(T, -1) != 0).repeat_interleave(int(n_agents), dim=1)
    g = torch.tensor(float(gamma), dtype=r.dtype, device=r.device)
    R = carry.reshape(-1).to(r.dtype).clone()
    sums = torch.zeros((2,), dtype=torch.float64, device=r.device)
    for t in range(T):
        R = R * g
        R = R + r[t]
        Rd = R.to(torch.float64)
        sums[0] += Rd.sum()
        sums[1] += (Rd * Rd).sum()
        if steps_out is not None:
            steps_out[t].copy_(R.reshape(steps_out[t].shape))
        R = torch.where(d[t], torch.zeros_like(R), R)
    return R, sums


class RetNorm:
    """Running variance of the discounted returns (VecNormalize's reward half,
    batched per rollout): the fp64 state (count, mean, m2) of every step's
    running return R, the fp32 per-column ``carry`` of R across rollouts, and
    the fp32 ``scale`` [1] = 1 / sqrt(m2 / count + eps) made from the state (1
    while the count is 0), all on `device`.  The mean is kept for the variance
    and never subtracted from a reward.  On a GPU ``update`` is mas_ret_stats +
    mas_obs_norm_merge with one column (include/masurvival.h); elsewhere the
    torch restatement (ret_stats_reference, merge_reference).  ``scale`` is
    updated in place and read on the device by mas_gae_scaled."""

    def __init__(self, n_columns, device, eps=1e-8):
        self.n_columns, self.device, self.eps = int(n_columns), torch.device(device), float(eps)
        self.state = torch.zeros((3,), dtype=torch.float64, device=self.device)
        self.batch = torch.zeros_like(self.state)
        self.carry = torch.zeros((self.n_columns,), dtype=torch.float32, device=self.device)
        self.scale = torch.ones((1,), dtype=torch.float32, device=self.device)
        self._mean32 = torch.zeros((1,), dtype=torch.float32, device=self.device)  # the merge's other output
        self._scratch = None
        self.lib = None
        if self.device.type == 'cuda':
            self.lib = load_library()
            if not hasattr(self.lib, 'mas_ret_stats') or not hasattr(self.lib, 'mas_obs_norm_merge'):
                raise MasError('the loaded library has no mas_ret_stats / mas_obs_norm_merge')

    @property
    def count(self):
        return self.state[0]

    def _merge(self, group, reduce):
        if reduce:
            dist.all_reduce(self.batch, group=group)
        if self.lib is not None:
            ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            check(self.lib.mas_obs_norm_merge(1, ptr(self.state), ptr(self.batch), self.eps, ptr(self._mean32),
                                              ptr(self.scale),
                                              ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        else:
            self.scale.copy_(merge_reference(self.state, self.batch, self.eps)[1])

    @torch.no_grad()
    def update(self, rewards, dones, n_agents, gamma, group=None, reduce=None, scratch=None):
        """Advance the carry through the rollout (rewards fp32 [T, columns..],
        dones uint8 [T, envs], column m of env m // n_agents) and merge its
        T * columns running returns into the state; `rewards` is only read.
        reduce (default: whether a group is given): all-reduce the batch
        record (count, sum, sum of squares) over `group` first, so every rank
        ends with the same state and scale (the carries stay per rank).
        scratch: a GPU caller's fp64 scratch to share (a gae_scratch of the
        same columns), for calls ordered on one stream."""
        T = rewards.shape[0]
        if rewards[0].numel() != self.n_columns or rewards.device.type != self.device.type:
            raise ValueError(f'RetNorm.update: need rewards of {self.n_columns} columns on {self.device}, got '
                             f'{tuple(rewards.shape)} on {rewards.device}')
        self.batch[:1].fill_(float(T * self.n_columns))  # (the all-reduce sums the ranks' counts in place)
        if self.lib is not None:
            if scratch is None:
                if self._scratch is None:
                    need = int(self.lib.mas_ret_stats_scratch_doubles(self.n_columns))
                    self._scratch = torch.empty((need,), dtype=torch.float64, device=self.device)
                scratch = self._scratch
            ret_stats(rewards, dones, gamma, self.carry, self.batch[1:], n_agents, scratch=scratch)
        else:
            carry, sums = ret_stats_reference(rewards, dones, gamma, self.carry, n_agents)
            self.carry.copy_(carry)
            self.batch[1:].copy_(sums)
        self._merge(group, group is not None if reduce is None else reduce)

    @torch.no_grad()
    def refresh(self):
        """scale again from the state (a merge of an empty batch)."""
        self.batch.zero_()
        self._merge(None, False)

    def state_dict(self):
        return {'count': self.state[0].detach().clone(), 'mean': self.state[1].detach().clone(),
                'm2': self.state[2].detach().clone(), 'eps': float(self.eps), 'carry': self.carry.detach().clone()}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if tuple(sd['carry'].shape) != (self.n_columns,):
            raise ValueError(f'RetNorm: checkpoint carry of shape {tuple(sd["carry"].shape)}, expected '
                             f'({self.n_columns},)')
        self.state[0] = sd['count'].to(torch.float64)
        self.state[1] = sd['mean'].to(torch.float64)
        self.state[2] = sd['m2'].to(torch.float64)
        self.carry.copy_(sd['carry'])
        self.eps = float(sd.get('eps', self.eps))
        self.refresh()

    @classmethod
    def from_state_dict(cls, sd, device):
        rn = cls(sd['carry'].numel(), device, sd.get('eps', 1e-8))
        rn.load_state_dict(sd)
        return rn


# the steps mas_episode_stats loads ahead of its recurrence in the default build
# (csrc/mas_epstats.hip MAS_EP_CHUNK).  Nothing computes with it: its tests place
# their rollout lengths around it, and under another chunk they only miss those edges
EPISODE_STATS_CHUNK = 8
# the record's integer entries, then sum_G[A] and sum_G2[A]
EPISODE_RECORD_HEAD = ('episodes', 'sum_len', 'sum_len2', 'wins0', 'wins1', 'draws')


def episode_stats_geometry():
    """(envs per workgroup, most agents per env) of mas_episode_stats in the
    loaded library, read off mas_episode_stats_scratch_doubles: 6 + 2A doubles
    per workgroup, -1 for an agent count the kernel does not take."""
    f = load_library().mas_episode_stats_scratch_doubles
    wg = 64
    while f(wg + 64, 1) == f(64, 1):
        wg += 64
    agents = 1
    while f(1, agents + 1) >= 0:
        agents += 1
    return wg, agents


def _episode_side_mask(side_mask, n_agents):
    m, A = int(side_mask), int(n_agents)
    if A < 1 or m < 0 or (m >> A) != 0:
        raise ValueError(f'episode statistics: side_mask {side_mask!r} has a bit at or above n_agents {n_agents}')
    return m


def _episode_stats_call(name, rewards, dones, n_agents, ret_carry, len_carry, record_out, side_mask, stream, scratch):
    """The checked mas_episode_stats call: its return code (ValueError for a wrong tensor first)."""
    lib = load_library()
    if not hasattr(lib, 'mas_episode_stats'):
        raise MasError('the loaded library has no mas_episode_stats')
    A = int(n_agents)
    mask = _episode_side_mask(side_mask, A)
    T, M = _rollout_columns(name, rewards, dones, A)
    E, dev = M // A, rewards.device
    for what, t, dtype, n in (('ret_carry', ret_carry, torch.float64, M), ('len_carry', len_carry, torch.int32, E),
                              ('record_out', record_out, torch.float64, len(EPISODE_RECORD_HEAD) + 2 * A)):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and t.is_contiguous()
                and t.numel() == n):
            raise ValueError(f'{name}: {what} must be a contiguous {dtype} tensor of {n} values on {dev}')
    need = int(lib.mas_episode_stats_scratch_doubles(E, A))
    if need < 0:
        raise ValueError(f'{name}: the kernel does not take {E} envs of {A} agents (episode_stats_reference does)')
    if scratch is None:
        scratch = torch.empty((need,), device=dev, dtype=torch.float64)
    if not (isinstance(scratch, torch.Tensor) and scratch.device == dev and scratch.dtype == torch.float64
            and scratch.is_contiguous() and scratch.numel() >= need):
        raise ValueError(f'{name}: scratch must hold {need} fp64 values on {dev}')
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return lib.mas_episode_stats(T, E, A, mask, ptr(rewards), ptr(dones), ptr(ret_carry), ptr(len_carry),
                                 ptr(record_out), ptr(scratch), ctypes.c_void_p(s))


def episode_stats(rewards, dones, n_agents, ret_carry, len_carry, record_out, side_mask=0, stream=None, scratch=None):
    """HIP episode statistics of a rollout (include/masurvival.h
    mas_episode_stats): rewards fp32 [T, N*A..] and dones uint8 [T, N] are
    walked forward per env from ret_carry (fp64 [N*A], each agent's return in
    the episode so far) and len_carry (int32 [N], its length so far), both
    advanced in place; record_out (fp64 [6 + 2A]) receives [episodes, sum_len,
    sum_len2, wins0, wins1, draws, sum_G[A], sum_G2[A]] over the episodes that
    ended in these T steps.  side_mask: the agents of side 0 (0 or all: no
    sides, no wins).  scratch: float64 device tensor of
    mas_episode_stats_scratch_doubles(N, A) (allocated here when None)."""
    check(_episode_stats_call('episode_stats', rewards, dones, n_agents, ret_carry, len_carry, record_out, side_mask,
                              stream, scratch))


def episode_stats_reference(rewards, dones, n_agents, ret_carry, len_carry, side_mask=0):
    """Plain torch restatement of mas_episode_stats with its order of
    operations per env (the CPU trainer's, and the fallback for more agents
    than the kernel takes): returns (the new ret_carry fp64 [N*A], the new
    len_carry int32 [N], the record fp64 [6 + 2A]).  The carries given are not
    written.  Across envs the terms are added in torch's order, not the
    kernel's: the integer entries agree exactly, the fp64 sums within rounding."""
    A = int(n_agents)
    mask = _episode_side_mask(side_mask, A)
    T = rewards.shape[0]
    r = rewards.reshape(T, -1, A)
    E, dev = r.shape[1], r.device
    d = dones.reshape(T, E) != 0
    G = ret_carry.reshape(E, A).to(torch.float64).clone()
    ln = len_carry.reshape(E).to(torch.int32).clone()
    rec = torch.zeros((len(EPISODE_RECORD_HEAD) + 2 * A,), dtype=torch.float64, device=dev)
    sides = mask != 0 and mask != (1 << A) - 1
    zG, zl, zE = torch.zeros_like(G), torch.zeros_like(ln), torch.zeros((E,), dtype=torch.float64, device=dev)
    for t in range(T):
        G = G + r[t].to(torch.float64)
        ln = ln + 1
        dt = d[t]
        L = ln.to(torch.float64)
        rec[0] += dt.sum()
        rec[1] += torch.where(dt, L, zE).sum()
        rec[2] += torch.where(dt, L * L, zE).sum()
        Gd = torch.where(dt[:, None], G, zG)
        rec[6:6 + A] += Gd.sum(0)
        rec[6 + A:] += (Gd * Gd).sum(0)
        if sides:
            s0, s1 = zE, zE
            for a in range(A):
                if (mask >> a) & 1:
                    s0 = s0 + G[:, a]
                else:
                    s1 = s1 + G[:, a]
            rec[3] += (dt & (s0 > s1)).sum()
            rec[4] += (dt & (s1 > s0)).sum()
            rec[5] += (dt & (s0 == s1)).sum()
        G = torch.where(dt[:, None], zG, G)
        ln = torch.where(dt, zl, ln)
    return G.reshape(-1), ln, rec


class EpisodeStats:
    """What the rollouts' finished episodes looked like (RecordEpisodeStatistics,
    batched per rollout): the per-env carries of every agent's undiscounted
    return (fp64 ``ret_carry`` [N*A]) and of the episode length (int32
    ``len_carry`` [N]) across rollouts, ``last`` (the record of the latest
    rollout, include/masurvival.h mas_episode_stats) and ``total`` (the sum of
    all records), fp64 on `device`.  On a GPU ``update`` is mas_episode_stats;
    elsewhere, and for a shape the kernel does not take (more agents per env
    than episode_stats_geometry() reports: mas_episode_stats_scratch_doubles is
    -1), the torch restatement.  Nothing is copied to the host before
    ``summary``."""

    def __init__(self, n_envs, n_agents, device, side_mask=0):
        self.n_envs, self.n_agents, self.device = int(n_envs), int(n_agents), torch.device(device)
        if self.n_envs < 1 or self.n_agents < 1:
            raise ValueError(f'EpisodeStats: need n_envs and n_agents >= 1, got {n_envs} and {n_agents}')
        self.side_mask = _episode_side_mask(side_mask, self.n_agents)
        n = len(EPISODE_RECORD_HEAD) + 2 * self.n_agents
        self.ret_carry = torch.zeros((self.n_envs * self.n_agents,), dtype=torch.float64, device=self.device)
        self.len_carry = torch.zeros((self.n_envs,), dtype=torch.int32, device=self.device)
        self.last = torch.zeros((n,), dtype=torch.float64, device=self.device)
        self.total = torch.zeros_like(self.last)
        self._scratch = None
        self.lib = None
        if self.device.type == 'cuda':
            self.lib = load_library()
            if not hasattr(self.lib, 'mas_episode_stats'):
                raise MasError('the loaded library has no mas_episode_stats')
            need = int(self.lib.mas_episode_stats_scratch_doubles(self.n_envs, self.n_agents))
            if need >= 0:
                self._scratch = torch.empty((need,), dtype=torch.float64, device=self.device)

    @torch.no_grad()
    def update(self, rewards, dones, group=None, reduce=None):
        """Walk one rollout (rewards fp32 [T, N, A], dones uint8 [T, N], only
        read): the carries advance, ``last`` becomes the rollout's record and
        is added to ``total``.  reduce (default: whether a group is given):
        all-reduce ``last`` over `group` first, so every rank ends with the
        same record (the carries stay per rank)."""
        if (rewards.dim() < 2 or rewards[0].numel() != self.n_envs * self.n_agents
                or rewards.device.type != self.device.type):
            raise ValueError(f'EpisodeStats.update: need rewards of {self.n_envs} x {self.n_agents} columns on '
                             f'{self.device}, got {tuple(rewards.shape)} on {rewards.device}')
        rc = MAS_ERR_UNSUPPORTED
        if self._scratch is not None:
            rc = _episode_stats_call('EpisodeStats.update', rewards, dones, self.n_agents, self.ret_carry,
                                     self.len_carry, self.last, self.side_mask, None, self._scratch)
        if rc == MAS_ERR_UNSUPPORTED:  # no GPU, no kernel for this shape, or refused with nothing launched
            G, ln, rec = episode_stats_reference(rewards, dones, self.n_agents, self.ret_carry, self.len_carry,
                                                 self.side_mask)
            self.ret_carry.copy_(G)
            self.len_carry.copy_(ln)
            self.last.copy_(rec)
        else:
            check(rc)
        if group is not None if reduce is None else reduce:
            dist.all_reduce(self.last, group=group)
        self.total += self.last

    def summary(self, which='last'):
        """Plain numbers from ``last`` or ``total`` (the one host copy):
        episodes, mean_length, std_length, return and return_std (a list per
        agent slot), wins (per side), draws, win_rate (side 0's).  Means are
        over the finished episodes; all 0 when none finished."""
        if which not in ('last', 'total'):
            raise ValueError(f"EpisodeStats.summary: which must be 'last' or 'total', got {which!r}")
        rec = getattr(self, which).tolist()
        A, n = self.n_agents, rec[0]
        k = 1.0 / n if n > 0 else 0.0
        mean_len = rec[1] * k
        ret = [g * k for g in rec[6:6 + A]]
        return {'episodes': int(n), 'mean_length': mean_len,
                'std_length': max(rec[2] * k - mean_len * mean_len, 0.0) ** 0.5,
                'return': ret,
                'return_std': [max(g2 * k - m * m, 0.0) ** 0.5 for g2, m in zip(rec[6 + A:], ret)],
                'wins': [int(rec[3]), int(rec[4])], 'draws': int(rec[5]), 'win_rate': rec[3] * k}

    def state_dict(self):
        return {'ret_carry': self.ret_carry.detach().clone(), 'len_carry': self.len_carry.detach().clone(),
                'last': self.last.detach().clone(), 'total': self.total.detach().clone(),
                'n_agents': int(self.n_agents), 'side_mask': int(self.side_mask)}

    @torch.no_grad()
    def load_state_dict(self, sd):
        have = (int(sd['n_agents']), tuple(sd['ret_carry'].shape), tuple(sd['len_carry'].shape),
                tuple(sd['last'].shape), tuple(sd['total'].shape), int(sd['side_mask']))
        want = (self.n_agents, tuple(self.ret_carry.shape), tuple(self.len_carry.shape), tuple(self.last.shape),
                tuple(self.total.shape), self.side_mask)
        if have != want:
            raise ValueError(f'EpisodeStats: checkpoint (n_agents, carry, length, record and total shapes, side_mask) '
                             f'{have}, expected {want}')
        self.ret_carry.copy_(sd['ret_carry'])
        self.len_carry.copy_(sd['len_carry'])
        self.last.copy_(sd['last'])
        self.total.copy_(sd['total'])

    @classmethod
    def from_state_dict(cls, sd, device):
        es = cls(sd['len_carry'].numel(), sd['n_agents'], device, sd['side_mask'])
        es.load_state_dict(sd)
        return es


def gae_reference(rewards, values, dones, gamma, lam, n_agents):
    """Plain torch restatement of mas_gae in the dtype of `rewards` (fp32: the
    CPU trainer's GAE; tests/gae_ref.py holds it to fp64).  Any nonzero done
    byte is done, as in the kernels."""
    T = rewards.shape[0]
    r = rewards.reshape(T, -1)
    v = values.reshape(T + 1, -1)
    nt = (dones.reshape(T, -1) == 0).to(r.dtype).repeat_interleave(n_agents, dim=1)
    adv = torch.zeros_like(r)
    a = torch.zeros_like(r[0])
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * v[t + 1] * nt[t] - v[t]
        a = delta + gamma * lam * nt[t] * a
        adv[t] = a
    return adv.reshape(rewards.shape), (adv + v[:T]).reshape(rewards.shape)


def gae_reference_into(rewards, values, dones, gamma, lam, adv_out, ret_out, sums_out, n_agents, stream=None,
                       scratch=None):
    """Same contract as gae() on host tensors -- test double for the CPU
    multi-process tests only (the product trainer always runs the HIP kernel)."""
    adv, ret = gae_reference(rewards, values, dones, gamma, lam, n_agents)
    adv_out.copy_(adv)
    ret_out.copy_(ret)
    sums_out[0] = adv.double().sum()
    sums_out[1] = (adv.double() ** 2).sum()


# MAS_POL_DW: the policy layers ('2', '3') whose weight gradients come from
# the mas_policy_dw kernel (LDS-staged split-K MFMA, k_dw_lds) instead of the
# split-K GEMMs (e.g. '23', '2', '0').  Per 4.2M-row minibatch (r02p7): layer
# 2 1.14 ms against 1.28 for its GEMM, layer 3 0.54 against 0.52 + the GEMM
# path's split-K sum; the update 30.3 ms with '2', 29.5 with '23'.
_DW_LAYERS = os.environ.get('MAS_POL_DW', '23')
# MAS_ACT_PAD: extra columns of the feature-major activation buffers (row
# stride M + pad; 0 = the power-of-two stride: dW2 kernel 1.21 vs 0.85 ms)
_ACT_PAD = int(os.environ.get('MAS_ACT_PAD', '64'))
# MAS_POL_LAYOUT: activation layout of the update ('fm' feature-major
# [F][rows] with the DPP row pairing and the mas_policy_dw kernels, 'rm'
# row-major [rows][F] written as plain 16-B stores, weight gradients as
# row-sum GEMMs)
_POL_LAYOUT = os.environ.get('MAS_POL_LAYOUT', 'fm')
_RM_LDH = 264  # row stride of the row-major h1 / h2 (column 256: ones)
# the train entry point of (form, row weights): layer 3 fused ('dw3'), stored
# feature-major ('fm'), row-major ('rm': no weighted form)
_TRAIN_FN = {('dw3', False): 'mas_policy_train_dw3', ('dw3', True): 'mas_policy_train_dw3_w',
             ('fm', False): 'mas_policy_train_ld', ('fm', True): 'mas_policy_train_w',
             ('rm', False): 'mas_policy_train_rm'}
# MAS_FUSED_ADAM=0: the torch clip_grad_norm_ + Adam step in the fused trainer
_FUSED_ADAM = os.environ.get('MAS_FUSED_ADAM', '1') != '0'


def _splitk_nt(a, b):
    """a [F, K] @ b[G, K]^T in fp32 for a huge K, as a batched GEMM over K
    chunks (bf16 in, partial sums reduced in fp32; rows may be strided)."""
    F_, K = a.shape
    G = b.shape[0]
    c = _split_k(K)
    pa = a.unflatten(1, (c, K // c)).permute(1, 0, 2)
    pb = b.unflatten(1, (c, K // c)).permute(1, 2, 0)
    return torch.bmm(pa, pb).sum(0, dtype=torch.float32)


def _splitk_tn(a, b):
    """a [K, F]^T @ b [K, G] in fp32 for a huge K (both row-major, any row
    stride): the row-sum GEMM of the row-major activations."""
    K = a.shape[0]
    c = _split_k(K)
    pa = a.unflatten(0, (c, K // c)).transpose(1, 2)
    pb = b.unflatten(0, (c, K // c))
    return torch.bmm(pa, pb).sum(0, dtype=torch.float32)


def _splitk_nn(a, x):
    """a [F, K] @ x [K, G] in fp32 for a huge K (x row-major, any row stride)."""
    F_, K = a.shape
    c = _split_k(K)
    pa = a.unflatten(1, (c, K // c)).permute(1, 0, 2)
    px = x.reshape(c, K // c, x.shape[1]) if x.is_contiguous() else x.unflatten(0, (c, K // c))
    return torch.bmm(pa, px).sum(0, dtype=torch.float32)


class FusedPolicy:
    """The HIP policy kernels (include/masurvival.h mas_policy_*) over a
    PolicyMLP's fp32 parameters: ``pack()`` after every optimizer step, ``act``
    for the rollout, ``grads`` for one PPO minibatch.  Hidden width 256."""

    def __init__(self, policy: 'PolicyMLP', obs_dim: int, device):
        self.lib = load_library()
        self.policy, self.D, self.device = policy, int(obs_dim), device
        self.Dp = 16 * ((self.D + 15) // 16)      # columns the kernels read / write
        self.Dx = 16 * ((self.D + 1 + 15) // 16)  # row stride of x: room for the bias column at index D
        w1, w2 = policy.body[0].weight, policy.body[2].weight
        assert w1.shape == (256, self.D) and w2.shape == (256, 256) and policy.head.weight.shape == (16, 256)
        self.packed = torch.empty((int(self.lib.mas_policy_packed_bytes(self.D)),), dtype=torch.uint8, device=device)
        self._bufs = None
        self._dwbuf = {}
        self.layout = _POL_LAYOUT
        if self.layout == 'rm':
            perm = [int(self.lib.mas_policy_rm_feature(c)) for c in range(256)]  # stored column -> feature
            q = [0] * 256
            for c, f in enumerate(perm):
                q[f] = c
            self._rm_q = torch.tensor(q, dtype=torch.long, device=device)  # feature -> stored column

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @torch.no_grad()
    def pack(self):
        p = self.policy
        ts = [p.body[0].weight, p.body[0].bias, p.body[2].weight, p.body[2].bias, p.head.weight, p.head.bias]
        ts = [t.detach().float().contiguous() for t in ts]
        if p.obs_mean is not None:
            # the input normaliser folded into layer 1 (mas_policy_pack_norm)
            if not hasattr(self.lib, 'mas_policy_pack_norm'):
                raise MasError('the loaded library has no mas_policy_pack_norm')
            ts += [p.obs_mean.detach().float().contiguous(), p.obs_inv_std.detach().float().contiguous()]
            check(self.lib.mas_policy_pack_norm(self.D, *[ctypes.c_void_p(t.data_ptr()) for t in ts],
                                                ctypes.c_void_p(self.packed.data_ptr()), self._stream()))
            return
        check(self.lib.mas_policy_pack(self.D, *[ctypes.c_void_p(t.data_ptr()) for t in ts],
                                       ctypes.c_void_p(self.packed.data_ptr()), self._stream()))

    def x_buffer(self, *shape):
        """bf16 policy-input rows [*shape, Dx] with the bias column (index D) = 1."""
        x = torch.zeros((*shape, self.Dx), dtype=torch.bfloat16, device=self.device)
        x[..., self.D] = 1.0
        return x

    @torch.no_grad()
    def act(self, obs, seed, step, actions, logp, value, xb=None, first_row=0):
        """obs [M, D] fp32 rows -> actions int8 [M, 6], logp, value [M];
        xb [M, Dx] bf16 (optional, from x_buffer) receives the rows as the
        update reads them.  first_row: index of obs[0] in the whole batch when
        the batch is launched in shards (the sampling RNG is keyed by it)."""
        M = obs.shape[0]
        assert obs.is_contiguous() and obs.dtype == torch.float32 and obs.shape[1] == self.D
        assert actions.is_contiguous() and logp.is_contiguous() and value.is_contiguous()
        xp = ctypes.c_void_p(xb.data_ptr()) if xb is not None else None
        check(self.lib.mas_policy_act_rows(ctypes.c_void_p(self.packed.data_ptr()), self.D, M, int(first_row),
                                           ctypes.c_void_p(obs.data_ptr()), xp, self.Dx, int(seed), int(step),
                                           ctypes.c_void_p(actions.data_ptr()), ctypes.c_void_p(logp.data_ptr()),
                                           ctypes.c_void_p(value.data_ptr()), self._stream()))

    @torch.no_grad()
    def act_x(self, xb, seed, step, actions, logp, value, first_row=0):
        """act over bf16 input rows xb [M, Dx] (x_buffer layout, e.g. written by
        mas_step_x): the same actions, log-probs and values as act on the fp32
        rows they were rounded from; xb is not written."""
        M = xb.shape[0]
        assert xb.is_contiguous() and xb.dtype == torch.bfloat16 and xb.shape[1] == self.Dx
        assert actions.is_contiguous() and logp.is_contiguous() and value.is_contiguous()
        check(self.lib.mas_policy_act_x(ctypes.c_void_p(self.packed.data_ptr()), self.D, M, int(first_row),
                                        ctypes.c_void_p(xb.data_ptr()), self.Dx, int(seed), int(step),
                                        ctypes.c_void_p(actions.data_ptr()), ctypes.c_void_p(logp.data_ptr()),
                                        ctypes.c_void_p(value.data_ptr()), self._stream()))

    @torch.no_grad()
    def act_sel(self, xb, n_agents, agent_mask, seed, step, actions, logp, value, greedy=False, logits=None,
                first_row=0):
        """act_x over the agents bit-selected by agent_mask of the whole envs in
        xb [n_envs * n_agents, Dx] (include/masurvival.h mas_policy_act_sel):
        only the selected agents' rows are read and only their rows of actions,
        logp, value (and logits fp32 [M, 16]: 15 logits, then the value) are
        written, with the values act_x gives them.  greedy: the first-index
        arg-max of every head instead of a draw (seed / step unused)."""
        M = xb.shape[0]
        assert xb.is_contiguous() and xb.dtype == torch.bfloat16 and xb.shape[1] == self.Dx
        assert actions.is_contiguous() and logp.is_contiguous() and value.is_contiguous()
        if not hasattr(self.lib, 'mas_policy_act_sel'):
            raise MasError('the loaded library has no mas_policy_act_sel')
        n_agents = int(n_agents)
        assert n_agents == 0 or M % n_agents == 0
        lp = None
        if logits is not None:
            assert logits.is_contiguous() and logits.dtype == torch.float32 and logits.shape == (M, 16)
            lp = ctypes.c_void_p(logits.data_ptr())
        check(self.lib.mas_policy_act_sel(ctypes.c_void_p(self.packed.data_ptr()), self.D,
                                          M // n_agents if n_agents > 0 else 0, n_agents, int(agent_mask),
                                          int(first_row), ctypes.c_void_p(xb.data_ptr()), self.Dx, int(seed),
                                          int(step), int(bool(greedy)), ctypes.c_void_p(actions.data_ptr()),
                                          ctypes.c_void_p(logp.data_ptr()), ctypes.c_void_p(value.data_ptr()), lp,
                                          self._stream()))

    def _buffers_rm(self, M):
        if self._bufs is None or self._bufs['M'] != M:
            bf = dict(dtype=torch.bfloat16, device=self.device)
            nb = int(self.lib.mas_policy_blocks(M))
            h1 = torch.zeros((M, _RM_LDH), **bf)
            h2 = torch.zeros((M, _RM_LDH), **bf)
            h1[:, 256] = 1.0
            h2[:, 256] = 1.0
            self._bufs = {'M': M, 'h1': h1, 'h2': h2, 'da1': torch.empty((M, 256), **bf),
                          'da2': torch.empty((M, 256), **bf), 'dz': torch.empty((M, 16), **bf),
                          'part': torch.empty((nb, 4), dtype=torch.float32, device=self.device)}
        return self._bufs

    def _train(self, form, xb, actions, old_logp, adv, ret, cfg, row_w, tail):
        """One call of the train entry point of `form` (_TRAIN_FN): the head all
        forms share, row_w where given, the coefficients, then the form's own
        tail (tensors as their pointers).  Returns the library's return code."""
        M = xb.shape[0]
        args = [self.packed, self.D, M, xb, self.Dx, actions, old_logp, adv, ret]
        args += ([row_w] if row_w is not None else []) + [cfg.clip, cfg.vf_coef, cfg.ent_coef, 1.0 / M, *tail]
        fn = getattr(self.lib, _TRAIN_FN[form, row_w is not None])
        return fn(*[ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args], self._stream())

    @staticmethod
    def _set_grads(grads):
        """.grad of every parameter in grads (None: already written in place)."""
        for prm, g in grads.items():
            if g is None:
                continue
            if prm.grad is None:
                prm.grad = g.to(prm.dtype).clone(memory_format=torch.contiguous_format)
            else:
                prm.grad.copy_(g)

    def _dw1(self, g1):
        """Layer 1's weight gradient from g1 = dA1 [x, 1] over the raw rows
        ([256, D + 1]): its first D columns, unfolded (unfold_dw1) when the
        policy carries an input normaliser -- the kernels differentiated the
        folded W1'.  In fp64, rounded once: g1w and g1b (x) mean nearly cancel in
        a column that sits far from zero."""
        p = self.policy
        if p.obs_mean is None:
            return g1[:, :self.D]
        return unfold_dw1(g1[:, :self.D].double(), g1[:, self.D].double(), p.obs_mean.double(),
                          p.obs_inv_std.double()).float()

    @staticmethod
    def _loss_stats(part, M, cfg):
        """(loss, pg, v, entropy, clipfrac) from the train kernel's partial records."""
        s = part.sum(0) / M
        pg, v, ent, clipfrac = s[0], s[1], s[2], s[3]
        return pg + cfg.vf_coef * v - cfg.ent_coef * ent, pg, v, ent, clipfrac

    def _grads_rm(self, xb, actions, old_logp, adv, ret, cfg):
        M = xb.shape[0]
        B = self._buffers_rm(M)
        check(self._train('rm', xb, actions, old_logp, adv, ret, cfg, None,
                          [B['h1'], B['h2'], _RM_LDH, B['da1'], B['da2'], B['dz'], B['part']]))
        q = self._rm_q
        g3 = _splitk_tn(B['dz'], B['h2'][:, :257])               # [16, 257], columns stored order
        g2 = _splitk_tn(B['da2'], B['h1'][:, :257])              # [256, 257]
        g1 = _splitk_tn(B['da1'], xb[:, :self.D + 1])            # [256, D + 1]
        g2 = g2.index_select(0, q)
        g1 = g1.index_select(0, q)
        p = self.policy
        l1, l2, l3 = p.body[0], p.body[2], p.head
        self._set_grads({l3.weight: g3[:, :256].index_select(1, q), l3.bias: g3[:, 256],
                         l2.weight: g2[:, :256].index_select(1, q), l2.bias: g2[:, 256],
                         l1.weight: self._dw1(g1), l1.bias: g1[:, self.D]})
        return self._loss_stats(B['part'], M, cfg)

    def _buffers(self, M):
        if self._bufs is None or self._bufs['M'] != M:
            bf = dict(dtype=torch.bfloat16, device=self.device)
            nb = int(self.lib.mas_policy_blocks(M))
            # h1 / h2 carry a row of ones (row 256): dW @ [h; 1]^T yields the bias gradient as its last column.
            # Row stride ld = M + _ACT_PAD: a power-of-two stride (the 4.2M-row minibatch) puts every
            # feature row on the same HBM channels (mas_policy_train_ld)
            ld = M + _ACT_PAD
            h1 = torch.empty((257, ld), **bf)
            h1[256] = 1.0
            # h2 / dz: _buffers_l3, only when a call stores them (mas_policy_train_dw3 does not)
            self._bufs = {'M': M, 'ld': ld, 'h1': h1,
                          'da1': torch.empty((256, ld), **bf), 'da2': torch.empty((256, ld), **bf),
                          'part': torch.empty((nb, 4), dtype=torch.float32, device=self.device)}
        return self._bufs

    def _buffers_l3(self, M):
        """_buffers(M) with the layer-3 activations h2 [257, ld] (row 256: ones)
        and dz [16, ld], which only the unfused path stores."""
        B = self._buffers(M)
        if 'h2' not in B:
            bf = dict(dtype=torch.bfloat16, device=self.device)
            B['h2'] = torch.empty((257, B['ld']), **bf)
            B['h2'][256] = 1.0
            B['dz'] = torch.empty((16, B['ld']), **bf)
        return B

    def _dw_buffers(self, F, M):
        """(split-K scratch, out [F * 256 + F]) of a layer's weight-gradient kernel."""
        key = ('dw', F, M)
        if key not in self._dwbuf:
            n = int(self.lib.mas_policy_dw_scratch(F, 256, M))
            self._dwbuf[key] = (torch.empty((n,), dtype=torch.float32, device=self.device),
                                torch.empty((F * 256 + F,), dtype=torch.float32, device=self.device))
        return self._dwbuf[key]

    def _dw(self, a, h, F, M, into=None):
        """(a[:, :M] @ h[:256, :M]^T, a.sum(1)) in fp32 via mas_policy_dw.
        into: (weight, bias) fp32 tensors that are one contiguous span of
        F * 256 + F floats (the flat gradient buffer of FusedAdam): the sums
        land there directly and (None, None) is returned."""
        scratch, out = self._dw_buffers(F, M)
        optr = into[0].data_ptr() if into is not None else out.data_ptr()
        check(self.lib.mas_policy_dw(F, 256, M, ctypes.c_void_p(a.data_ptr()), a.stride(0), ctypes.c_void_p(h.data_ptr()),
                                     h.stride(0), ctypes.c_void_p(optr), ctypes.c_void_p(scratch.data_ptr()),
                                     self._stream()))
        if into is not None:
            return None, None
        return out[:F * 256].view(F, 256), out[F * 256:]

    @staticmethod
    def _grad_span(w, b):
        """(w.grad, b.grad) when they are one contiguous fp32 span, weight then
        bias (FusedAdam's flat buffer), else None."""
        gw, gb = w.grad, b.grad
        if gw is None or gb is None or gw.dtype != torch.float32 or gb.dtype != torch.float32:
            return None
        if not (gw.is_contiguous() and gb.is_contiguous()):
            return None
        if gw.untyped_storage().data_ptr() != gb.untyped_storage().data_ptr():
            return None
        if gb.data_ptr() != gw.data_ptr() + 4 * gw.numel():
            return None
        return gw, gb

    def grads(self, xb, actions, old_logp, adv, ret, cfg: 'PPOConfig', stats: bool = True, row_w=None):
        """Sets .grad of the policy parameters to the gradient of the PPO loss
        (mean over the M rows) and returns (loss, pg, v, entropy, clipfrac);
        stats=False skips those reductions (the update keeps only the last
        minibatch's) and returns None.  row_w: fp32 [M] weights (>= 0) of the
        rows' policy terms (include/masurvival.h mas_policy_train_w); pg,
        entropy and clipfrac are then sum(w * term) / M."""
        M = xb.shape[0]
        assert xb.dtype == torch.bfloat16 and xb.shape[1] == self.Dx and xb.is_contiguous()
        for t in (actions, old_logp, adv, ret):
            assert t.is_contiguous()
        if row_w is not None:
            if self.layout == 'rm':
                raise ValueError('row weights need the feature-major layout (MAS_POL_LAYOUT=fm): the row-major '
                                 'train kernel has no weighted form')
            if not hasattr(self.lib, 'mas_policy_train_w'):
                raise MasError('the loaded library has no mas_policy_train_w')
            assert row_w.dtype == torch.float32 and row_w.shape == (M,) and row_w.is_contiguous()
            assert row_w.device == xb.device
        if self.layout == 'rm':
            return self._grads_rm(xb, actions, old_logp, adv, ret, cfg)
        p = self.policy
        l1, l2, l3 = p.body[0], p.body[2], p.head
        # layer 3 inside the train kernel (mas_policy_train_dw3: h2 and dz are
        # not stored) where the library takes the minibatch that way
        fused3 = False
        if '3' in _DW_LAYERS and hasattr(self.lib, _TRAIN_FN['dw3', row_w is not None]):
            B = self._buffers(M)
            span3 = self._grad_span(l3.weight, l3.bias)
            scratch3, out3 = self._dw_buffers(16, M)
            rc = self._train('dw3', xb, actions, old_logp, adv, ret, cfg, row_w,
                             [B['h1'], B['da1'], B['da2'], B['ld'], B['part'],
                              span3[0] if span3 is not None else out3, scratch3])
            if rc != MAS_ERR_UNSUPPORTED:  # refused (nothing written): the unfused path below
                check(rc)
                fused3 = True
        if not fused3:
            B = self._buffers_l3(M)
            check(self._train('fm', xb, actions, old_logp, adv, ret, cfg, row_w,
                              [B['h1'], B['h2'], B['da1'], B['da2'], B['dz'], B['ld'], B['part']]))
        B = {k: (v[:, :M] if k in ('h1', 'h2', 'da1', 'da2', 'dz') else v) for k, v in B.items()}
        # layers 2 / 3: the split-K MFMA kernel (mas_policy_dw) where enabled,
        # else the split-K GEMM over the ones-row trick; layer 1 reads x
        # row-major: a GEMM.  With FusedAdam's flat gradient buffer the dW
        # kernels' sums land in .grad directly (no copy launches)
        if fused3:
            g3w, g3b = (None, None) if span3 is not None else (out3[:16 * 256].view(16, 256), out3[16 * 256:])
        elif '3' in _DW_LAYERS and M % 32 == 0:
            g3w, g3b = self._dw(B['dz'], B['h2'], 16, M, into=self._grad_span(l3.weight, l3.bias))
        else:
            g3 = _splitk_nt(B['dz'], B['h2'])          # [16, 257]
            g3w, g3b = g3[:, :256], g3[:, 256]
        if '2' in _DW_LAYERS and M % 32 == 0:
            g2w, g2b = self._dw(B['da2'], B['h1'], 256, M, into=self._grad_span(l2.weight, l2.bias))
        else:
            g2 = _splitk_nt(B['da2'], B['h1'])         # [256, 257]
            g2w, g2b = g2[:, :256], g2[:, 256]
        g1 = _splitk_nn(B['da1'], xb[:, :self.D + 1])  # [256, D + 1]
        # (a None gradient: written in place above)
        self._set_grads({l3.weight: g3w, l3.bias: g3b, l2.weight: g2w, l2.bias: g2b,
                         l1.weight: self._dw1(g1), l1.bias: g1[:, self.D]})
        return self._loss_stats(B['part'], M, cfg) if stats else None


def masked_mean(x, row_w=None):
    """mean(x), or mean(w * x) over all rows where the rows with w == 0 do
    not count whatever x holds there (inf, NaN): a selection, as the kernels'.
    (The selection guards the value only: autograd through it still multiplies
    the dropped branch's derivative by zero, so what x is computed from must
    be finite there -- surrogate_terms.)"""
    if row_w is None:
        return x.mean()
    return torch.where(row_w != 0, row_w * x, torch.zeros_like(x)).mean()


def surrogate_terms(lp, old_logp, adv, clip, row_w=None):
    """(clipped surrogate min(r A, clip(r) A) per row, ratio r).  With row_w
    the rows with w == 0 take log-ratio 0 and advantage 0 before the
    exponential, so that neither their value nor their derivative can be
    inf or NaN whatever old_logp and adv hold there."""
    d = lp - old_logp
    if row_w is not None:
        live = row_w != 0
        d = torch.where(live, d, torch.zeros_like(d))
        adv = torch.where(live, adv, torch.zeros_like(adv))
    ratio = torch.exp(d)
    return torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv), ratio


def policy_loss_reference(policy, x, actions, old_logp, adv, ret, cfg: 'PPOConfig', row_w=None):
    """Plain torch fp32 restatement of the PPO loss the fused kernels
    differentiate (the numerics tests' reference): x fp32 rows [M, D].
    row_w: fp32 [M] weights of the rows' surrogate and entropy terms
    (mas_policy_train_w); the value term is never weighted."""
    logits, v = policy(x)
    lp, ent = evaluate_actions(logits, actions)
    pg = masked_mean(-surrogate_terms(lp, old_logp, adv, cfg.clip, row_w)[0], row_w)
    vl = F.mse_loss(v, ret)
    em = masked_mean(ent, row_w)
    return pg + cfg.vf_coef * vl - cfg.ent_coef * em, pg, vl, em


def chunk_row_weights(active, chunks):
    """(row_w shaped like active, share [chunks]) for `active` (fp32 0 / 1,
    any shape) cut into `chunks` equal contiguous minibatches: row_w = active
    * rows / sum(active) per chunk, zeros where a chunk has no active row (no
    NaN); share = the chunk's fraction of active rows.  On the tensor's
    device, no host synchronisation."""
    a = active.reshape(chunks, -1)
    rows = a.shape[1]
    n = a.sum(1, dtype=torch.float64)
    f = torch.where(n > 0, rows / n.clamp_min(1.0), torch.zeros_like(n)).float()
    return (a * f.unsqueeze(1)).reshape(active.shape), (n / rows).float()


class FusedAdam:
    """clip_grad_norm_ + torch.optim.Adam.step() for the fused trainer as one
    HIP launch pair (include/masurvival.h mas_policy_adam).  The parameters,
    their gradients and both Adam moments become views into four flat fp32
    buffers; the torch.optim.Adam object keeps holding them as its state, so
    its state_dict (checkpoints) is unchanged.  bind_state() re-points that
    state after Adam.load_state_dict replaced it.

    Used only for the plain form it restates (supports()): one param group,
    a float lr, no weight decay, amsgrad, maximize or capturable state; any
    other optimizer setup stays on torch.  After step(), ``.grad`` of each
    parameter holds the raw summed minibatch gradient the kernel read (the
    1 / world scale and the clip are applied inside the kernel, not written
    back), unlike torch's clip_grad_norm_, which scales .grad in place."""

    @staticmethod
    def supports(opt) -> bool:
        if not isinstance(opt, torch.optim.Adam) or len(opt.param_groups) != 1:
            return False
        g = opt.param_groups[0]
        return (not g.get('weight_decay', 0) and not g.get('amsgrad', False) and not g.get('maximize', False)
                and not g.get('capturable', False) and not g.get('differentiable', False)
                and not isinstance(g['lr'], torch.Tensor))

    def __init__(self, params, opt: torch.optim.Adam, lib, device):
        self.params, self.opt, self.lib, self.device = list(params), opt, lib, device
        n = sum(p.numel() for p in self.params)
        f = dict(dtype=torch.float32, device=device)
        self.p, self.g = torch.empty((n,), **f), torch.zeros((n,), **f)
        self.m, self.v = torch.zeros((n,), **f), torch.zeros((n,), **f)
        self.scratch = torch.empty((int(lib.mas_policy_adam_scratch()),), **f)
        self.spans = []
        off = 0
        with torch.no_grad():
            for prm in self.params:
                k = prm.numel()
                self.p[off:off + k].copy_(prm.detach().reshape(-1))
                prm.data = self.p[off:off + k].view_as(prm)
                prm.grad = self.g[off:off + k].view_as(prm)
                self.spans.append((off, k))
                off += k
        self.bind_state()

    @torch.no_grad()
    def bind_state(self):
        for prm, (off, k) in zip(self.params, self.spans):
            st = self.opt.state[prm]
            if 'exp_avg' in st:
                self.m[off:off + k].copy_(st['exp_avg'].reshape(-1))
                self.v[off:off + k].copy_(st['exp_avg_sq'].reshape(-1))
            else:
                self.m[off:off + k].zero_()
                self.v[off:off + k].zero_()
                st['step'] = torch.tensor(0.0)
            st['exp_avg'] = self.m[off:off + k].view_as(prm)
            st['exp_avg_sq'] = self.v[off:off + k].view_as(prm)

    def step(self, max_norm: float, grad_scale: float = 1.0):
        grp = self.opt.param_groups[0]
        steps = [self.opt.state[prm]['step'] for prm in self.params]
        for t in steps:
            t += 1  # CPU scalars, as torch.optim.Adam keeps them
        b1, b2 = grp['betas']
        check(self.lib.mas_policy_adam(self.p.numel(), ctypes.c_void_p(self.p.data_ptr()),
                                       ctypes.c_void_p(self.g.data_ptr()), ctypes.c_void_p(self.m.data_ptr()),
                                       ctypes.c_void_p(self.v.data_ptr()), float(grad_scale), float(max_norm),
                                       float(grp['lr']), float(b1), float(b2), float(grp['eps']),
                                       int(steps[0].item()), ctypes.c_void_p(self.scratch.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))


class RolloutBuffer:
    def __init__(self, T, N, A, D, device, with_obs=True):
        self.T, self.N, self.A, self.D = T, N, A, D
        f = dict(device=device, dtype=torch.float32)
        self.obs = torch.zeros((T + 1, N, A, D), **f) if with_obs else None
        self.actions = torch.zeros((T, N, A, 6), device=device, dtype=torch.int8)
        self.logp = torch.zeros((T, N, A), **f)
        self.values = torch.zeros((T + 1, N, A), **f)
        self.rewards = torch.zeros((T, N, A), **f)
        self.dones = torch.zeros((T, N), device=device, dtype=torch.uint8)
        self.adv = torch.zeros((T, N, A), **f)
        self.ret = torch.zeros((T, N, A), **f)
        # [sum, sum of squares, count] of the advantages: mas_gae writes the
        # sums into the first two (adv_sums is that view), the count is set
        # here (no host copy per iteration)
        self.adv_stats = torch.zeros((3,), device=device, dtype=torch.float64)
        self.adv_stats[2] = float(T * N * A)
        self.adv_sums = self.adv_stats[:2]
        self.gae_scratch = None  # mas_gae's partial sums (made at the first HIP GAE call)
        self.xb = None  # fused path: bf16 policy-input rows [T (+1 with x_obs), N*A, Dx] (mas_policy_act / mas_step_x)
        # self-play: the learner's rows of this rollout, compacted once per
        # iteration into a buffer of the same shape with A = its agent count
        # (alloc_learner); GAE and the update then read only that one
        self.learner = None
        # PPOConfig.mask_dead (alloc_active): the agents' alive flags before
        # each step, fp32 [T, N, A]; per iteration the minibatch weights made
        # from them (chunk_row_weights) and each minibatch's active share
        self.active = None
        self.row_w = None
        self.active_share = None

    def alloc_active(self, device):
        self.active = torch.ones((self.T, self.N, self.A), device=device, dtype=torch.float32)
        return self.active

    def alloc_learner(self, m, device, fused=None):
        """The dense buffer of m learner agents per env: the fields GAE and the
        update read, `dones` shared with this buffer; on the fused path bf16
        rows xb [T, N*m, Dx] instead of fp32 obs."""
        lb = RolloutBuffer(self.T, self.N, m, self.D, device, with_obs=fused is None)
        lb.dones = self.dones
        if fused is not None:
            lb.xb = fused.x_buffer(self.T, self.N * m)
        if self.active is not None:
            lb.alloc_active(device)
        self.learner = lb
        return lb


def _allreduce_grads(params, world, group=None):
    """One flat bucket (~0.5 MB for the 2x256 MLP): a single RCCL ring
    all-reduce per minibatch instead of one per parameter tensor."""
    grads = [p.grad for p in params]
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, group=group)
    flat.div_(world)
    off = 0
    for g in grads:
        n = g.numel()
        g.copy_(flat[off:off + n].view_as(g))
        off += n


class PPOTrainer:
    """Collect T steps of every env on this rank, GAE on device, PPO update.

    Fused path (GPU, hidden 256, the default there): the rollout step is ONE
    HIP kernel (mas_policy_act: MLP forward + sampling, also storing the bf16
    policy input for the update); each PPO minibatch is one HIP kernel
    (mas_policy_train: forward, loss gradient, backward data path) plus three
    split-K weight-gradient GEMMs.  Minibatches are contiguous time chunks of
    the rollout (T/minibatches steps of every env), visited in a random order
    each epoch: no row gather.  The torch path (random row minibatches,
    autograd) serves the CPU tests and is the numerics reference."""

    def __init__(self, env, cfg: PPOConfig = PPOConfig(), seed: int = 0, group=None, opponent=None,
                 learner_agents=None):
        """opponent: a frozen policy (a PolicyMLP, a checkpoint path or a
        loaded checkpoint dict, as match.load_policy reads them) that drives
        the agents outside `learner_agents`; the trained policy acts for and is
        updated on the rows of `learner_agents` only (default with an
        opponent: range(n_agents // 2), Match's side 0).  Both None: every
        agent is the trained policy's and nothing below changes.
        opponent may also be a scripted bot (masurvival.bots: a Bot or a
        'bot:NAME' string): it fills the other agents' action rows by its fixed
        rule (mas_bot_act on a GPU); it is kept as `opponent_bot`, `opponent`
        stays None, and there is nothing to sync."""
        from .bots import is_bot_spec, parse_bot
        self.env, self.cfg = env, cfg
        self.device = env.device
        self.opponent_bot = parse_bot(opponent) if is_bot_spec(opponent) else None
        if self.opponent_bot is not None:
            if int(cfg.opponent_sync_every) > 0:
                raise ValueError('opponent_sync_every > 0 needs a policy opponent: a bot has no weights to sync')
            if getattr(env, 'rc', None) is None:
                raise ValueError('a bot opponent needs the env config (an env with .rc)')
            self._bot_cfg = env.rc.to_struct()
            opponent = None
        self.opponent, self.learner_agents = self._resolve_selfplay(env, opponent, learner_agents,
                                                                    self.opponent_bot is not None)
        self.group = group
        self.world = dist.get_world_size(group) if group is not None or dist.is_initialized() else 1
        self.collectives = self.world > 1 if cfg.allreduce is None else bool(cfg.allreduce)
        if self.collectives and not (group is not None or dist.is_initialized()):
            raise ValueError('PPOConfig.allreduce=True needs an initialised torch.distributed process group')
        torch.manual_seed(seed)  # identical init on every rank
        self.policy = PolicyMLP(env.obs_dim, cfg.hidden).to(self.device)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=cfg.lr, eps=1e-5)
        self.buf = RolloutBuffer(cfg.horizon, env.n_envs, env.n_agents, env.obs_dim, self.device)
        if cfg.mask_dead:
            if not callable(getattr(env, 'alive', None)):
                raise ValueError(f'PPOConfig.mask_dead needs an env with alive() ({type(env).__name__} has none)')
            self.buf.alloc_active(self.device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed * 7919 + (dist.get_rank() if dist.is_initialized() else 0))
        self.buf.obs[0].copy_(env.reset())
        self.last_stats = {}
        self.iterations = 0  # finished iteration() calls (opponent_sync_every)
        self.opp_fused = None
        self.gae_impl = gae  # the HIP kernel; CPU tests inject gae_reference_into
        self.seed = int(seed) * 1000003 + (dist.get_rank() if dist.is_initialized() else 0)
        self.steps_taken = 0
        self._rollout_policy = None
        # the input normaliser (ObsNorm), attached to the policy; also made by
        # load_state_dict from a checkpoint that has one.  cfg.obs_norm only
        # decides whether it keeps updating
        self.obs_norm = None
        if cfg.obs_norm:
            self._attach_obs_norm(ObsNorm(env.obs_dim, self.device, cfg.obs_norm_eps))
        # the reward normaliser (RetNorm) over the columns GAE reads (with
        # self-play the learner's); also made by load_state_dict from a
        # checkpoint that has one.  Its scale is applied whenever it exists;
        # cfg.reward_norm only decides whether it keeps updating
        self.ret_norm = None
        if cfg.reward_norm:
            if not (cfg.reward_clip > 0):
                raise ValueError(f'PPOConfig.reward_clip must be positive (inf: no clipping), got {cfg.reward_clip}')
            self.ret_norm = RetNorm(self._gae_columns(), self.device, cfg.reward_norm_eps)
        # the episode statistics (EpisodeStats) over the whole buffer, every agent's columns under
        # self-play too; also made by load_state_dict from a checkpoint that has them.
        # cfg.episode_stats only decides whether they keep updating
        self.ep_stats = None
        if cfg.episode_stats:
            self.ep_stats = EpisodeStats(env.n_envs, env.n_agents, self.device, self._side0_mask())
        fused = cfg.fused
        if fused is None:
            fused = self.device.type == 'cuda' and cfg.hidden == 256
        self.fused = None
        self.fused_opt = None
        self.x_obs = False
        if fused:
            self.fused = FusedPolicy(self.policy, env.obs_dim, self.device)
            b = self.buf
            xo = cfg.x_obs
            if xo is None:
                # MAS_X_OBS=0 in the environment: the fp32 obs path (A/B runs)
                xo = (os.environ.get('MAS_X_OBS', '1') != '0' and hasattr(env, 'supports_step_x')
                      and env.supports_step_x())
            self.x_obs = bool(xo)
            # x_obs: rows T + 1 (the env writes step t's next rows into t + 1)
            self.buf.xb = self.fused.x_buffer(b.T + (1 if self.x_obs else 0), b.N * b.A)
            if self.x_obs:
                self._set_x0(self.buf.obs[0])
            M = b.N * b.A
            self._boot = (torch.empty((M, 6), dtype=torch.int8, device=self.device),
                          torch.empty((M,), dtype=torch.float32, device=self.device))
            if cfg.obs_norm:
                self._obs_norm_merge_reset()  # the first rollout is already scaled
            self.fused.pack()
            if cfg.mask_dead and self.fused.layout == 'rm':
                raise ValueError('PPOConfig.mask_dead needs the feature-major update (MAS_POL_LAYOUT=fm)')
            if _FUSED_ADAM and FusedAdam.supports(self.opt):
                self.fused_opt = FusedAdam(self.policy.parameters(), self.opt, self.fused.lib, self.device)
        else:
            if cfg.obs_norm:
                self._obs_norm_merge_reset()
            self._sync_rollout_policy()
        if self.learner_agents is not None:
            self._init_selfplay()

    def _gae_columns(self):
        """Agent columns of the buffer GAE reads: every agent's, with self-play the learner's."""
        A = self.env.n_agents if self.learner_agents is None else len(self.learner_agents)
        return int(self.env.n_envs) * int(A)

    def _has_opponent(self):
        return self.opponent is not None or self.opponent_bot is not None

    def _side0_mask(self):
        """Side 0 of the episode statistics: the learner's agents against an
        opponent, otherwise agents range(A // 2) (Match's side 0; none for one agent)."""
        A = int(self.env.n_agents)
        side0 = self.learner_agents if self._has_opponent() else range(A // 2)
        return _agent_mask(side0, A, 'side 0') if len(side0) else 0

    def _episode_last_stats(self):
        """last_stats' share of the latest rollout's record: device tensors, means over max(episodes, 1)."""
        rec, A = self.ep_stats.last, self.ep_stats.n_agents
        n = rec[0].clamp_min(1.0)
        return {'episodes': rec[0].clone(), 'ep_length': rec[1] / n, 'ep_return': rec[6:6 + A] / n,
                'win_rate': rec[3] / n}

    def episode_summary(self, which='total'):
        """EpisodeStats.summary of the training rollouts' episodes (plain numbers; a host copy)."""
        if self.ep_stats is None:
            raise ValueError('episode_summary: this trainer keeps no episode statistics (PPOConfig.episode_stats)')
        return self.ep_stats.summary(which)

    def _attach_obs_norm(self, on):
        self.obs_norm = on
        self.policy.set_obs_norm(on.mean, on.inv_std)

    @torch.no_grad()
    def _obs_norm_merge_reset(self):
        """Merge time block 0, the reset rows (with self-play the learner's),
        before the first rollout; they count again as block 0 of that rollout."""
        b = self.buf
        if self.x_obs:
            rows = b.xb[0].view(b.N, b.A, -1)
        else:
            rows = b.obs[0].to(torch.bfloat16)  # rounded as the kernels round
        if self.learner_agents is not None:
            rows = rows[:, self.learner_agents]
        self._obs_norm_update(rows.reshape(-1, rows.shape[-1]), kernel=self.x_obs)

    def _obs_norm_update(self, rows, kernel):
        """rows bf16 [M, >= D] into the normaliser: mas_obs_stats where the
        rows are the kernels' (kernel), else the torch restatement; the batch
        record all-reduced first when this trainer runs collectives."""
        if kernel:
            self.obs_norm.update(rows.contiguous(), group=self.group, reduce=self.collectives)
        else:
            self.obs_norm.update_reference(rows, group=self.group, reduce=self.collectives)

    @torch.no_grad()
    def _obs_norm_after_update(self):
        """Merge the rows the update has just trained on (blocks [0, T); with
        self-play the learner's dense rows), before block 0 is overwritten; the
        callers then pack / sync, so the next rollout and its update see the
        new normaliser and a first minibatch's ratios stay 1."""
        full, T = self.buf, self.cfg.horizon
        b = full if full.learner is None else full.learner
        if self.fused is not None:
            self._obs_norm_update(b.xb[:T].view(-1, self.fused.Dx), kernel=True)
        else:
            self._obs_norm_update(b.obs[:T].reshape(-1, b.D).to(torch.bfloat16), kernel=False)

    @staticmethod
    def _resolve_selfplay(env, opponent, learner_agents, bot=False):
        """(frozen opponent PolicyMLP or None, sorted learner agent list or
        None) from the constructor's arguments, or ValueError.  bot: a scripted
        bot stands where the opponent would (opponent is None then)."""
        if opponent is None and learner_agents is None and not bot:
            return None, None
        A = int(env.n_agents)
        if not 1 <= A <= 32:
            raise ValueError(f'self-play: n_agents {A} outside 1..32')
        if learner_agents is None:
            learner_agents = range(A // 2)
        learner_agents = [int(a) for a in learner_agents]
        _agent_mask(learner_agents, A, 'learner_agents')
        whole = len(learner_agents) == A
        if bot:
            if whole:
                raise ValueError('learner_agents must be a proper subset of the agents when an opponent is given')
            return None, sorted(learner_agents)
        if opponent is None:
            if not whole:
                raise ValueError(f'learner_agents {learner_agents} leaves agents without a policy: give an opponent')
            return None, sorted(learner_agents)
        if whole:
            raise ValueError('learner_agents must be a proper subset of the agents when an opponent is given')
        if isinstance(opponent, PolicyMLP):
            import copy
            opponent = copy.deepcopy(opponent)
        else:
            from .match import load_policy  # (match imports this module)
            opponent = load_policy(opponent)
        d = int(opponent.body[0].weight.shape[1])
        if d != env.obs_dim:
            raise ValueError(f'opponent obs_dim {d} does not match the env obs_dim {env.obs_dim}')
        opponent = opponent.to(env.device).float().eval()
        for p in opponent.parameters():
            p.requires_grad_(False)
        return opponent, sorted(learner_agents)

    def _init_selfplay(self):
        b, A = self.buf, self.buf.A
        self._lmask = _agent_mask(self.learner_agents, A)
        self._omask = ((1 << A) - 1) ^ self._lmask
        self._lidx = torch.tensor(self.learner_agents, dtype=torch.long, device=self.device)
        self._lsel = torch.zeros((A,), dtype=torch.bool, device=self.device)
        self._lsel[self._lidx] = True
        if self.device.type == 'cuda':
            why = None
            if self.fused is None:
                why = 'the fused policy kernels (PPOConfig.fused, hidden 256)'
            elif not self.x_obs:
                why = 'the bf16-row rollout (PPOConfig.x_obs, an env with step_x)'
            elif hasattr(self.env, 'shard_slices'):
                why = 'an unsharded env'
            if why is not None:
                raise ValueError(f'self-play on a GPU needs {why}')
            if not hasattr(self.fused.lib, 'mas_rows_select') or not hasattr(self.fused.lib, 'mas_policy_act_sel'):
                raise MasError('the loaded library has no mas_rows_select / mas_policy_act_sel')
            if self.opponent_bot is not None and not hasattr(self.fused.lib, 'mas_bot_act'):
                raise MasError('the loaded library has no mas_bot_act')
            if self.opponent is not None:
                self.opp_fused = FusedPolicy(self.opponent, self.env.obs_dim, self.device)
                self.opp_fused.pack()
                # the opponent's log-probs and values: written, never read
                self._opp_out = (torch.empty((b.N * A,), dtype=torch.float32, device=self.device),
                                 torch.empty((b.N * A,), dtype=torch.float32, device=self.device))
        elif self.fused is not None:
            raise ValueError('self-play with the fused kernels needs a GPU env')
        b.alloc_learner(len(self.learner_agents), self.device, self.fused)

    @torch.no_grad()
    def sync_opponent(self):
        """Lagged self-play: the opponent becomes a copy of the learner's
        current fp32 weights (and is packed again for the kernels)."""
        if self.opponent_bot is not None:
            raise ValueError(f'sync_opponent: the opponent is the bot {self.opponent_bot.name!r}, which has no weights')
        if self.opponent is None:
            raise ValueError('sync_opponent: this trainer has no opponent')
        for d, s_ in zip(self.opponent.parameters(), self.policy.parameters()):
            d.copy_(s_)
        # (a copy of the normaliser as it is now: the learner's keeps moving)
        mean, inv_std = self.policy.obs_mean, self.policy.obs_inv_std
        self.opponent.set_obs_norm(*((None, None) if mean is None else (mean.clone(), inv_std.clone())))
        if self.opp_fused is not None:
            self.opp_fused.pack()

    @torch.no_grad()
    def _set_x0(self, obs):
        """x_obs: the first rollout rows from fp32 obs [N, A, D] (a reset's,
        or a checkpoint's): rounded to bf16 as the kernels round."""
        b = self.buf
        b.xb[0][:, :b.D].copy_(obs.reshape(-1, b.D).to(torch.bfloat16))

    def _fwd(self, x, policy=None):
        with torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=self.cfg.autocast_bf16):
            return (self.policy if policy is None else policy)(x)

    @torch.no_grad()
    def _sync_rollout_policy(self):
        """bf16 copy of the policy for the rollout forward (refreshed after each
        update): no per-step weight casts under autocast."""
        if self.cfg.autocast_bf16 and self.device.type == 'cuda':
            if self._rollout_policy is None:
                import copy
                self._rollout_policy = copy.deepcopy(self.policy).to(torch.bfloat16)
            for d, s_ in zip(self._rollout_policy.parameters(), self.policy.parameters()):
                d.copy_(s_)
            if self.policy.obs_mean is not None:
                self._rollout_policy.set_obs_norm(self.policy.obs_mean.to(torch.bfloat16),
                                                  self.policy.obs_inv_std.to(torch.bfloat16))

    @torch.no_grad()
    def _rollout_step_selfplay(self, t):
        """One step with the learner on its agents and the opponent (when
        there is one) on the others: both fill the same actions[t]."""
        b = self.buf
        if b.active is not None:
            self.env.alive(out=b.active[t])
        if self.fused is not None:
            acts = b.actions[t].view(-1, 6)
            # one RNG key for both calls: it is keyed by the physical row
            self.fused.act_sel(b.xb[t], b.A, self._lmask, self.seed, self.steps_taken, acts, b.logp[t].view(-1),
                               b.values[t].view(-1))
            if self.opp_fused is not None:
                self.opp_fused.act_sel(b.xb[t], b.A, self._omask, self.seed, self.steps_taken, acts, *self._opp_out)
            elif self.opponent_bot is not None:
                from .bots import bot_act
                bot_act(self._bot_cfg, self.opponent_bot, b.xb[t], b.A, self._omask, acts)
            self.steps_taken += 1
            self.env.step_x(b.actions[t], b.xb[t + 1], b.rewards[t], b.dones[t])
            return
        logits, v = self._fwd(b.obs[t])
        a, lp = sample_actions(logits, self.gen)
        if self.opponent is not None:
            ao, _ = sample_actions(self._fwd(b.obs[t], self.opponent)[0], self.gen)
            a = torch.where(self._lsel.view(1, -1, 1), a, ao)
        elif self.opponent_bot is not None:
            from .bots import bot_actions_reference
            ao = bot_actions_reference(self.opponent_bot, b.obs[t], self._bot_cfg)
            a = torch.where(self._lsel.view(1, -1, 1), a, ao.to(a.dtype))
        b.actions[t].copy_(a)
        b.logp[t].copy_(lp)
        b.values[t].copy_(v)
        self.steps_taken += 1
        self.env.step(b.actions[t], out=(b.obs[t + 1], b.rewards[t], b.dones[t]))

    @torch.no_grad()
    def _select_learner_rows(self):
        """The learner's rows of the finished rollout into buf.learner."""
        b, lb = self.buf, self.buf.learner
        T = b.T
        if self.fused is not None:
            Dx = self.fused.Dx
            rows_select(b.A, self._lmask, x=b.xb[:T].view(-1, Dx), x_out=lb.xb.view(-1, Dx),
                        actions=b.actions.view(-1, 6), actions_out=lb.actions.view(-1, 6),
                        f32=[(b.logp, lb.logp), (b.rewards, lb.rewards)]
                        + ([(b.active, lb.active)] if b.active is not None else []))
            rows_select(b.A, self._lmask, f32=[(b.values, lb.values)])  # T + 1 row blocks
            return
        i = self._lidx
        lb.obs[:T].copy_(b.obs[:T].index_select(2, i))
        lb.actions.copy_(b.actions.index_select(2, i))
        lb.logp.copy_(b.logp.index_select(2, i))
        lb.rewards.copy_(b.rewards.index_select(2, i))
        lb.values.copy_(b.values.index_select(2, i))
        if b.active is not None:
            lb.active.copy_(b.active.index_select(2, i))

    @torch.no_grad()
    def rollout_step(self, t):
        b = self.buf
        if self.learner_agents is not None:
            return self._rollout_step_selfplay(t)
        if self.fused is not None and hasattr(self.env, 'shard_slices'):
            # sharded env (vec_env.ShardedVecMaSurvival): each shard's policy
            # forward + env step on its own stream, so one shard's act
            # overlaps the others' env kernels; rows keep their global RNG key
            A, D = b.A, b.D
            self.env.fork()
            for e, s, lo, hi in self.env.shard_slices():
                with torch.cuda.stream(s):
                    r0, r1 = lo * A, hi * A
                    if b.active is not None:
                        e.alive(out=b.active[t][lo:hi])
                    if self.x_obs:
                        self.fused.act_x(b.xb[t][r0:r1], self.seed, self.steps_taken,
                                         b.actions[t].view(-1, 6)[r0:r1], b.logp[t].view(-1)[r0:r1],
                                         b.values[t].view(-1)[r0:r1], first_row=r0)
                        e.step_x(b.actions[t][lo:hi], b.xb[t + 1][r0:r1], b.rewards[t][lo:hi], b.dones[t][lo:hi])
                        continue
                    self.fused.act(b.obs[t].view(-1, D)[r0:r1], self.seed, self.steps_taken,
                                   b.actions[t].view(-1, 6)[r0:r1], b.logp[t].view(-1)[r0:r1],
                                   b.values[t].view(-1)[r0:r1], xb=b.xb[t][r0:r1], first_row=r0)
                    e.step(b.actions[t][lo:hi], out=(b.obs[t + 1][lo:hi], b.rewards[t][lo:hi], b.dones[t][lo:hi]))
            self.env.join()
            self.steps_taken += 1
            return
        if b.active is not None:
            self.env.alive(out=b.active[t])  # the agents whose actions this step reads
        if self.x_obs:
            # the env wrote these rows (bf16) at the last step; it writes the
            # next ones into row block t + 1
            self.fused.act_x(b.xb[t], self.seed, self.steps_taken, b.actions[t].view(-1, 6), b.logp[t].view(-1),
                             b.values[t].view(-1))
            self.steps_taken += 1
            self.env.step_x(b.actions[t], b.xb[t + 1], b.rewards[t], b.dones[t])
            return
        if self.fused is not None:
            self.fused.act(b.obs[t].view(-1, b.D), self.seed, self.steps_taken, b.actions[t].view(-1, 6),
                           b.logp[t].view(-1), b.values[t].view(-1), xb=b.xb[t])
        elif self.device.type == 'cuda':
            if self._rollout_policy is not None:
                h = self._rollout_policy.forward_raw(b.obs[t].to(torch.bfloat16))  # [N, A, 16] fp32
            else:
                h = self.policy.forward_raw(b.obs[t])
            h2 = h.reshape(-1, N_LOGITS + 1)
            sample_actions_hip(h2, self.seed, self.steps_taken, b.actions[t].view(-1, 6), b.logp[t].view(-1))
            b.values[t].copy_(h[..., N_LOGITS])
        else:  # CPU stand-in tests
            logits, v = self._fwd(b.obs[t])
            a, lp = sample_actions(logits, self.gen)
            b.actions[t].copy_(a)
            b.logp[t].copy_(lp)
            b.values[t].copy_(v)
        self.steps_taken += 1
        self.env.step(b.actions[t], out=(b.obs[t + 1], b.rewards[t], b.dones[t]))

    @torch.no_grad()
    def finish_rollout(self):
        b, c = self.buf, self.cfg
        if self.learner_agents is not None and self.fused is not None:
            self.fused.act_sel(b.xb[c.horizon], b.A, self._lmask, self.seed, 0, self._boot[0], self._boot[1],
                               b.values[c.horizon].view(-1))
        elif self.x_obs:
            self.fused.act_x(b.xb[c.horizon], self.seed, 0, self._boot[0], self._boot[1], b.values[c.horizon].view(-1))
        elif self.fused is not None:
            self.fused.act(b.obs[c.horizon].view(-1, b.D), self.seed, 0, self._boot[0], self._boot[1],
                           b.values[c.horizon].view(-1))
        else:
            _, v = self._fwd(b.obs[c.horizon])
            b.values[c.horizon].copy_(v)
        if self.ep_stats is not None and c.episode_stats:
            # every agent's rewards of the whole buffer, before the learner's rows are selected
            self.ep_stats.update(b.rewards, b.dones, group=self.group, reduce=self.collectives)
        if b.learner is not None:
            # self-play: GAE, the statistics and the update see the learner's rows alone
            self._select_learner_rows()
            b = b.learner
        if self.gae_impl is gae and b.gae_scratch is None:
            b.gae_scratch = gae_scratch(b.N * b.A, self.device)
        rn = self.ret_norm
        if rn is not None and c.reward_norm:
            # this rollout's running returns into the statistics before its rewards are scaled (as
            # VecNormalize updates before it normalises); the calls share the GAE scratch: one stream
            rn.update(b.rewards, b.dones, b.A, c.gamma, group=self.group, reduce=self.collectives,
                      scratch=b.gae_scratch)
        if rn is None:
            self.gae_impl(b.rewards, b.values, b.dones, c.gamma, c.lam, b.adv, b.ret, b.adv_sums, b.A,
                          scratch=b.gae_scratch)
        elif self.gae_impl is gae:
            # the scale applied where GAE loads the reward, read from device memory; b.rewards stays raw
            gae_scaled(b.rewards, b.values, b.dones, c.gamma, c.lam, rn.scale, c.reward_clip, b.adv, b.ret,
                       b.adv_sums, b.A, scratch=b.gae_scratch)
        else:
            # the CPU path and the injected test double: the kernel's two fp32 steps on a copy
            self.gae_impl(scale_rewards_reference(b.rewards, rn.scale, c.reward_clip), b.values, b.dones, c.gamma,
                          c.lam, b.adv, b.ret, b.adv_sums, b.A, scratch=b.gae_scratch)
        stats = b.adv_stats  # (b.adv_sums is its first two entries)
        if b.active is not None:
            # the statistics over the active rows: (sum w adv, sum w adv^2, sum w) in double (w is 0 or 1);
            # a rollout without any active row keeps a count of 1 (its weights are all zero anyway)
            # (the reductions accumulate in double from the fp32 products: no fp64 copy of the rollout)
            wa = b.active * b.adv
            stats[0].copy_(wa.sum(dtype=torch.float64))
            stats[1].copy_(torch.linalg.vector_norm(wa, 2, dtype=torch.float64).square())
            stats[2].copy_(b.active.sum(dtype=torch.float64).clamp_min(1.0))
            del wa
            b.row_w, b.active_share = chunk_row_weights(b.active, c.minibatches if self.fused is not None else 1)
        if self.collectives:
            if b.active is None:
                stats[2].fill_(float(b.adv.numel()))  # the all-reduce below sums the counts in place
            dist.all_reduce(stats, group=self.group)
        if self.gae_impl is gae and b.adv.is_cuda:
            # one launch (include/masurvival.h mas_adv_normalize), the roundings of the expression below
            adv_normalize(b.adv, stats)
        else:
            mean = stats[0] / stats[2]
            var = (stats[1] / stats[2] - mean * mean).clamp_min(0.0)
            b.adv.sub_(mean.float()).div_(var.sqrt().float() + 1e-8)

    def _update_fused(self):
        full, c = self.buf, self.cfg
        b = full if full.learner is None else full.learner  # self-play: the learner's dense rows
        assert c.horizon % c.minibatches == 0, 'fused update: horizon must split into whole time chunks'
        tc = c.horizon // c.minibatches
        params = list(self.policy.parameters())
        for ep in range(c.epochs):
            order = torch.randperm(c.minibatches, generator=torch.Generator().manual_seed(self.steps_taken))
            for n, k in enumerate(order.tolist()):
                sl = slice(k * tc, (k + 1) * tc)
                xb = b.xb[sl].reshape(-1, self.fused.Dx)
                M = xb.shape[0]
                # last_stats keeps the last minibatch's loss terms: only it reduces them
                last = ep == c.epochs - 1 and n == c.minibatches - 1
                rw = None if b.row_w is None else b.row_w[sl].reshape(M)
                st = self.fused.grads(xb, b.actions[sl].reshape(M, 6), b.logp[sl].reshape(M),
                                      b.adv[sl].reshape(M), b.ret[sl].reshape(M), c, stats=last, row_w=rw)
                if last:
                    loss, pg, vl, ent, cf = st
                    share = None if b.active_share is None else b.active_share[k]
                if self.fused_opt is not None:
                    # flat gradient buffer: one all-reduce, the 1 / world folded into the step
                    if self.collectives:
                        dist.all_reduce(self.fused_opt.g, group=self.group)
                    self.fused_opt.step(c.max_grad_norm, 1.0 / self.world if self.collectives else 1.0)
                else:
                    if self.collectives:
                        _allreduce_grads(params, self.world, self.group)
                    nn.utils.clip_grad_norm_(params, c.max_grad_norm)
                    self.opt.step()
                self.fused.pack()
        self.last_stats = {'loss': loss.detach(), 'pg': pg.detach(), 'v': vl.detach(), 'entropy': ent.detach(),
                           'clipfrac': cf.detach()}
        if share is not None:
            self.last_stats['active'] = share
        if c.reward_norm:
            self.last_stats['reward_scale'] = self.ret_norm.scale[0].clone()
        if c.episode_stats:
            self.last_stats.update(self._episode_last_stats())
        if c.obs_norm:
            self._obs_norm_after_update()
            self.fused.pack()
        if self.x_obs:
            full.xb[0].copy_(full.xb[c.horizon])
        else:
            full.obs[0].copy_(full.obs[c.horizon])

    def update(self):
        if self.fused is not None:
            return self._update_fused()
        full, c = self.buf, self.cfg
        b = full if full.learner is None else full.learner  # self-play: the learner's dense rows
        M = c.horizon * b.N * b.A
        obs = b.obs[:c.horizon].reshape(M, b.D)
        acts = b.actions.reshape(M, 6)
        old_lp, adv, ret = b.logp.reshape(M), b.adv.reshape(M), b.ret.reshape(M)
        params = list(self.policy.parameters())
        mb = M // c.minibatches
        active = None if b.active is None else b.active.reshape(M)
        for _ in range(c.epochs):
            perm = torch.randperm(M, device=self.device, generator=self.gen)
            for k in range(c.minibatches):
                idx = perm[k * mb:(k + 1) * mb]
                logits, v = self._fwd(obs[idx])
                lp, ent = evaluate_actions(logits, acts[idx])
                # mask_dead: this minibatch's weights (its rows are a random draw: made here)
                rw, share = (None, None) if active is None else chunk_row_weights(active[idx], 1)
                pg = masked_mean(-surrogate_terms(lp, old_lp[idx], adv[idx], c.clip, rw)[0], rw)
                vl = F.mse_loss(v, ret[idx])
                loss = pg + c.vf_coef * vl - c.ent_coef * masked_mean(ent, rw)
                self.opt.zero_grad(set_to_none=False)
                loss.backward()
                if self.collectives:
                    _allreduce_grads(params, self.world, self.group)
                nn.utils.clip_grad_norm_(params, c.max_grad_norm)
                self.opt.step()
        self.last_stats = {'loss': loss.detach(), 'pg': pg.detach(), 'v': vl.detach()}
        if share is not None:
            self.last_stats['active'] = share[0]
        if c.reward_norm:
            self.last_stats['reward_scale'] = self.ret_norm.scale[0].clone()
        if c.episode_stats:
            self.last_stats.update(self._episode_last_stats())
        if c.obs_norm:
            self._obs_norm_after_update()
        self._sync_rollout_policy()
        full.obs[0].copy_(full.obs[c.horizon])

    # -- checkpoint / resume ------------------------------------------------
    # The reference has no trainer (SURVEY.md §5 lists checkpointing as an
    # auxiliary); this keeps what a resumed run needs to continue the same
    # trajectory: fp32 master weights, Adam moments, the sampling counters and
    # generator, the next rollout's first observation and, when the env exposes
    # mas_get_state (VecMaSurvival), the whole batched env state.  Only tensors
    # and plain numbers, so torch.load(weights_only=True) reads it back.

    def state_dict(self):
        sd = {'policy': self.policy.state_dict(), 'opt': self.opt.state_dict(),
              'steps_taken': int(self.steps_taken), 'seed': int(self.seed),
              'gen': self.gen.get_state(), 'obs0': self.buf.obs[0].detach().clone()}
        if self.x_obs:
            sd['xb0'] = self.buf.xb[0].detach().clone()  # (x_obs: the next rollout's rows; obs0 is the reset's)
        if self.obs_norm is not None:
            sd['obs_norm'] = self.obs_norm.state_dict()  # three fp64 tensors and eps (match.load_policy reads it)
        if self.ret_norm is not None:
            sd['ret_norm'] = self.ret_norm.state_dict()  # count, mean, m2 (fp64), eps and the columns' carry
        if self.ep_stats is not None:
            sd['ep_stats'] = self.ep_stats.state_dict()  # the carries, the last record and the lifetime total
        if self.learner_agents is not None:
            # self-play: 'policy' stays the learner (match.load_policy reads it as any checkpoint's)
            sd['learner_agents'] = [int(a) for a in self.learner_agents]
            sd['iterations'] = int(self.iterations)
            if self.opponent_bot is not None:
                sd['opponent_bot'] = self.opponent_bot.name
            if self.opponent is not None:
                sd['opponent'] = {k: v.detach().clone() for k, v in self.opponent.state_dict().items()}
                if self.opponent.obs_mean is not None:  # the frozen normaliser as the opponent applies it
                    sd['opponent_obs_norm'] = {'mean': self.opponent.obs_mean.detach().clone(),
                                               'inv_std': self.opponent.obs_inv_std.detach().clone()}
        if hasattr(self.env, 'get_state'):
            sd['env'] = self.env.get_state().detach().clone()
            if hasattr(self.env, 'state_meta'):
                sd['env_meta'] = self.env.state_meta()
        elif hasattr(self.env, 'n_envs') and self.env.__class__.__module__.startswith('masurvival'):
            raise ValueError(f'{type(self.env).__name__} cannot export its env state (no get_state): '
                             'a checkpoint without it would not resume the same trajectory')
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        have = sd.get('learner_agents')
        if (None if have is None else [int(a) for a in have]) != self.learner_agents:
            raise ValueError(f'checkpoint learner_agents {have} differ from this trainer\'s {self.learner_agents}')
        have_bot, my_bot = sd.get('opponent_bot'), (None if self.opponent_bot is None else self.opponent_bot.name)
        if have_bot != my_bot:
            raise ValueError(f'checkpoint opponent bot {have_bot!r} differs from this trainer\'s {my_bot!r}')
        if ('opponent' in sd) != (self.opponent is not None):
            raise ValueError('checkpoint and trainer disagree on having an opponent')
        if self.opponent is not None:
            self.opponent.load_state_dict(sd['opponent'])
            on = sd.get('opponent_obs_norm')
            self.opponent.set_obs_norm(*((None, None) if on is None else
                                         (on['mean'].to(self.device).float(), on['inv_std'].to(self.device).float())))
            if self.opp_fused is not None:
                self.opp_fused.pack()
        self.iterations = int(sd.get('iterations', 0))
        self.policy.load_state_dict(sd['policy'])
        if 'obs_norm' in sd:
            # restored whatever cfg.obs_norm says: the flag only decides whether it keeps updating
            if self.obs_norm is None:
                self._attach_obs_norm(ObsNorm(self.env.obs_dim, self.device, self.cfg.obs_norm_eps))
            self.obs_norm.load_state_dict(sd['obs_norm'])
        if 'ret_norm' in sd:
            # restored (and its scale applied) whatever cfg.reward_norm says; a checkpoint without one
            # leaves a flagged trainer's fresh statistics as they are
            if self.ret_norm is None:
                self.ret_norm = RetNorm(self._gae_columns(), self.device, self.cfg.reward_norm_eps)
            self.ret_norm.load_state_dict(sd['ret_norm'])
        if 'ep_stats' in sd:
            # restored whatever cfg.episode_stats says; a checkpoint without them leaves a flagged
            # trainer's fresh statistics as they are
            if self.ep_stats is None:
                self.ep_stats = EpisodeStats(self.env.n_envs, self.env.n_agents, self.device,
                                             self._side0_mask())
            self.ep_stats.load_state_dict(sd['ep_stats'])
        self.opt.load_state_dict(sd['opt'])
        if self.fused_opt is not None:
            self.fused_opt.bind_state()
        self.steps_taken = int(sd['steps_taken'])
        self.seed = int(sd['seed'])
        self.gen.set_state(sd['gen'].cpu())  # generator states are CPU ByteTensors (map_location moves them)
        if 'env' in sd:
            if not hasattr(self.env, 'set_state'):
                raise ValueError('checkpoint holds an env state but this env has no set_state')
            want = sd.get('env_meta')
            have = self.env.state_meta() if hasattr(self.env, 'state_meta') else None
            if want is not None and have is not None:
                # a state image only means something for the same config,
                # capacity class, env count and shard split
                diff = {k: (want.get(k), have.get(k)) for k in have if want.get(k) != have.get(k)}
                if diff:
                    raise ValueError(f'checkpoint env state does not match this env: {diff}')
            self.env.set_state(sd['env'].to(self.device))
        self.buf.obs[0].copy_(sd['obs0'])
        if self.x_obs:
            if 'xb0' in sd:
                self.buf.xb[0].copy_(sd['xb0'])
            else:
                self._set_x0(self.buf.obs[0])
        if self.fused is not None:
            self.fused.pack()
        else:
            self._sync_rollout_policy()

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location=self.device, weights_only=True))

    def iteration(self):
        with _phase('mas.rollout'):
            for t in range(self.cfg.horizon):
                self.rollout_step(t)
        with _phase('mas.gae'):
            self.finish_rollout()
        with _phase('mas.update'):
            self.update()
        self.iterations += 1
        k = int(self.cfg.opponent_sync_every)
        if self.opponent is not None and k > 0 and self.iterations % k == 0:
            self.sync_opponent()
