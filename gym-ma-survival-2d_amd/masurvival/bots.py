"""Scripted baseline opponents: fixed rules that act from the observation rows.

``mas_bot_act`` (include/masurvival.h holds the rule's normative text) fills
the action rows of the bit-selected agents on the device, from the same bf16
rows the policies read: the slot of ``mas_policy_act_sel`` with no network.
``Match`` and ``PPOTrainer(opponent='bot:NAME')`` put a bot where a policy can
stand; ``bot_actions_reference`` is the torch / fp64 stand-in for the CPU, as
``gae_reference`` is for its kernel.

    idle     never acts (the no-op row)
    hunter   walks into the zone, then at the nearest visible living enemy, and hits it
    forager  walks into the zone, collects heals inside it, fights only within 4 m

Every bot uses a heal it carries once its health has room for it.
"""
from __future__ import annotations

import ctypes

import torch

from .abi import MasError, check, load_library
from .layout import obs_layout

BOT_KINDS = {'idle': 0, 'hunter': 1, 'forager': 2}  # MAS_BOT_IDLE, MAS_BOT_HUNTER, MAS_BOT_FORAGER
BOT_PREFIX = 'bot:'

# the constants of the rule (include/masurvival.h)
_ZONE_MARGIN, _TURN_BAND, _TURN_DAMP = 1.0, 0.15, 0.25
_MOVE_CONE, _ATTACK_CONE, _STANDOFF, _ARRIVED, _FORAGER_FIGHT = 0.8, 0.9, 1.25, 0.25, 4.0


class Bot:
    """A scripted opponent by name; ``kind`` is its MAS_BOT_* number."""

    def __init__(self, name: str):
        name = str(name)
        if name not in BOT_KINDS:
            raise ValueError(f'unknown bot {name!r}: one of {sorted(BOT_KINDS)}')
        self.name, self.kind = name, BOT_KINDS[name]

    def __repr__(self):
        return f'Bot({self.name!r})'

    def __eq__(self, other):
        return isinstance(other, Bot) and other.name == self.name

    def __hash__(self):
        return hash(('Bot', self.name))


def is_bot_spec(spec) -> bool:
    """True for a Bot and for a 'bot:...' string (whatever name follows)."""
    return isinstance(spec, Bot) or (isinstance(spec, str) and spec.startswith(BOT_PREFIX))


def parse_bot(spec) -> Bot:
    """'bot:hunter' -> Bot('hunter'); a Bot passes through.  ValueError for a
    string without the prefix or with an unknown name."""
    if isinstance(spec, Bot):
        return spec
    if not isinstance(spec, str) or not spec.startswith(BOT_PREFIX):
        raise ValueError(f'not a bot: {spec!r} (expected {BOT_PREFIX}NAME, NAME one of {sorted(BOT_KINDS)})')
    return Bot(spec[len(BOT_PREFIX):])


def _kind_of(kind) -> int:
    if isinstance(kind, Bot):
        return kind.kind
    if isinstance(kind, str):
        return parse_bot(kind if kind.startswith(BOT_PREFIX) else BOT_PREFIX + kind).kind
    return int(kind)


def _struct_of(config):
    return config.to_struct() if hasattr(config, 'to_struct') else config


@torch.no_grad()
def bot_act(cfg_struct, kind, x, n_agents, agent_mask, actions, stream=None):
    """mas_bot_act over x bf16 [n_envs * n_agents, Dx] (a policy's row buffer):
    the rows of the agents in agent_mask get their 6 bytes of actions int8
    [n_envs * n_agents, 6]; nothing else is read or written.  Stream-ordered on
    `stream` (default: torch's current stream of x's device)."""
    lib = load_library()
    if not hasattr(lib, 'mas_bot_act'):
        raise MasError('the loaded library has no mas_bot_act')
    if not (x.is_cuda and actions.is_cuda):
        raise ValueError('bot_act needs device tensors (on the CPU: bot_actions_reference)')
    n_agents = int(n_agents)
    if n_agents != int(cfg_struct.n_agents):
        raise ValueError(f'n_agents {n_agents} differs from the config\'s {int(cfg_struct.n_agents)}')
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.bfloat16
    M = x.shape[0]
    assert M % n_agents == 0
    assert actions.is_contiguous() and actions.dtype == torch.int8 and actions.numel() == M * 6
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    check(lib.mas_bot_act(ctypes.byref(cfg_struct), _kind_of(kind), M // n_agents, int(agent_mask),
                          ctypes.c_void_p(x.data_ptr()), int(x.shape[1]), ctypes.c_void_p(actions.data_ptr()),
                          ctypes.c_void_p(int(stream))))
    return actions


def _nearest(d2, valid):
    """(index of the least d2 among valid, the lowest index among equals; any valid)."""
    big = torch.where(valid, d2, torch.full_like(d2, float('inf')))
    # argmin does not promise the first of equal minima: take it explicitly
    least = big.min(dim=1, keepdim=True).values
    n = d2.shape[1]
    idx = torch.arange(n, device=d2.device).expand_as(d2)
    k = torch.where(big == least, idx, torch.full_like(idx, n)).min(dim=1).values.clamp_max(n - 1)
    return k, valid.any(dim=1)


@torch.no_grad()
def bot_actions_reference(kind, obs, resolved_config):
    """The rule of mas_bot_act in torch fp64: obs [..., >= obs_dim] (fp32 or
    bf16 rows) -> actions int8 [..., 6].  The stand-in where there is no GPU;
    on bf16 rows it equals the kernel except where a comparison falls within
    fp32 rounding of its threshold."""
    kind = _kind_of(kind)
    if kind not in BOT_KINDS.values():
        raise ValueError(f'unknown bot kind {kind}')
    cs = _struct_of(resolved_config)
    A, H, teams = int(cs.n_agents), int(cs.n_heals), int(bool(cs.teams))
    D, lay = obs_layout(A, H, int(cs.n_boxes), bool(teams), int(cs.lidar_n_lasers))
    if obs.shape[-1] < D:
        raise ValueError(f'rows of {obs.shape[-1]} columns, the config\'s obs_dim is {D}')
    rows = obs.reshape(-1, obs.shape[-1]).to(torch.float64)
    R, dev = rows.shape[0], rows.device
    out = torch.zeros((R, 6), dtype=torch.int8, device=dev)
    out[:, :3] = 1
    if kind == BOT_KINDS['idle'] or R == 0:
        return out.reshape(*obs.shape[:-1], 6)
    rec, o = 8 + teams, 1 + teams
    ag = lay['agent'][0]
    hp, px, py, th, w = (rows[:, ag + o + k] for k in (0, 1, 2, 3, 6))
    zo = lay['zone'][0]
    zx, zy, zr = rows[:, zo], rows[:, zo + 1], rows[:, zo + 2]
    live = hp > 0
    use = torch.zeros_like(live)
    if H > 0:
        use = live & (rows[:, lay['heal_slot_mask'][0]] == 0) & (hp <= float(int(cs.agent_health) - int(cs.healing)))
    m = (zr - _ZONE_MARGIN).clamp_min(0.0)
    m2 = m * m
    tk = ((px - zx) ** 2 + (py - zy) ** 2 > m2).to(torch.int64)  # 0 none, 1 zone, 2 heal, 3 enemy
    tx, ty = torch.where(tk == 1, zx, torch.zeros_like(zx)), torch.where(tk == 1, zy, torch.zeros_like(zy))
    ar = torch.arange(R, device=dev)
    if kind == BOT_KINDS['forager'] and H > 0:
        h0 = lay['heals'][0]
        hs = rows[:, h0:h0 + 2 * H].reshape(R, H, 2)
        hm = lay['heals_mask'][0]
        ok = (rows[:, hm:hm + H] == 0) & ~((hs[:, :, 0] - zx[:, None]) ** 2 + (hs[:, :, 1] - zy[:, None]) ** 2
                                          > m2[:, None])
        k, has = _nearest((hs[:, :, 0] - px[:, None]) ** 2 + (hs[:, :, 1] - py[:, None]) ** 2, ok)
        take = (tk == 0) & has
        tk = torch.where(take, torch.full_like(tk, 2), tk)
        tx, ty = torch.where(take, hs[ar, k, 0], tx), torch.where(take, hs[ar, k, 1], ty)
    o0 = lay['others'][0]
    ot = rows[:, o0:o0 + (A - 1) * rec].reshape(R, A - 1, rec)
    om = lay['others_mask'][0]
    ok = (rows[:, om:om + A - 1] == 0) & (ot[:, :, o] > 0)
    if teams:
        ok &= ot[:, :, 1] != rows[:, ag + 1][:, None]
    d2 = (ot[:, :, o + 1] - px[:, None]) ** 2 + (ot[:, :, o + 2] - py[:, None]) ** 2
    k, has = _nearest(d2, ok)
    take = (tk == 0) & has
    if kind == BOT_KINDS['forager']:
        take &= ~(d2[ar, k] > _FORAGER_FIGHT * _FORAGER_FIGHT)
    tk = torch.where(take, torch.full_like(tk, 3), tk)
    tx, ty = torch.where(take, ot[ar, k, o + 1], tx), torch.where(take, ot[ar, k, o + 2], ty)

    dx, dy = tx - px, ty - py
    ln = torch.sqrt(dx * dx + dy * dy)
    hx, hy = torch.cos(th), torch.sin(th)
    c, s = hx * dx + hy * dy, hx * dy - hy * dx
    u, b = s - (_TURN_DAMP * w) * ln, _TURN_BAND * ln
    one, two, zero = torch.ones_like(tk), torch.full_like(tk, 2), torch.zeros_like(tk)
    turn = torch.where(u > b, two, torch.where(-b > u, zero, torch.where(0.0 > c, two, one)))
    enemy = tk == 3
    stop = torch.where(enemy, torch.full_like(ln, _STANDOFF), torch.full_like(ln, _ARRIVED))
    move = torch.where((c > _MOVE_CONE * ln) & (ln > stop), two, one)
    reach = float(cs.melee_range) + float(cs.agent_size) / 2.0
    hit = enemy & ~(ln > reach) & (c > _ATTACK_CONE * ln)
    has_t = tk != 0
    out[:, 0] = torch.where(has_t, move, one).to(torch.int8)
    out[:, 2] = torch.where(has_t, turn, two).to(torch.int8)
    out[:, 3] = (has_t & hit).to(torch.int8)
    out[:, 4] = use.to(torch.int8)
    out[~live] = torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.int8, device=dev)
    return out.reshape(*obs.shape[:-1], 6)
