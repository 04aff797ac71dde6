// mas_bot.hip -- mas_bot_act (include/masurvival.h): scripted baseline
// opponents.  Fills the action rows of the bit-selected agents from their bf16
// observation rows by the rule of mas_bot_rule.h; no network, no random
// numbers, no LDS, no scratch, every offset 64-bit.
//
// kGroup = 8 lanes share a row (8 rows per wave, 32 per workgroup).  The
// fields the rule reads are scattered over the row (the agent record at its
// start, heal_slot_mask .. zone in its last ~100 B at 2v2), so one lane per
// row would touch 64 different rows per load instruction.  Here
//   * lane g of a group loads header fields g and g + 8 (health, x, y, angle,
//     w, team, zone x, y, r, heal_slot_mask) and the group broadcasts them
//     with width-8 shuffles: two loads per lane instead of ten;
//   * candidate q = g, g + 8, ... of the row's [others | heals] list is lane
//     g's: its record's fields sit next to the neighbour lanes' in the same
//     row, so a load instruction touches 8 rows' lines, not 64 (2v2 has
//     3 + 4 = 7 candidates: one pass);
//   * every lane keeps its nearest admissible (enemy, heal) and three xor
//     shuffles reduce them over the group under the total order of
//     bot::nearer (squared distance, then index), so the result does not
//     depend on which lane held what;
//   * every lane of the group evaluates bot::decide on the same values (the
//     wave executes it once either way) and lane 0 stores the row's 6 bytes as
//     three 2-B words.
// A group past the last row works on the last row again (valid addresses, no
// branch around the loads) and stores nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mas_bot_rule.h"

namespace mas {
namespace bot {

constexpr int kThreads = 256;
constexpr int kGroup = 8;
constexpr int kRowsPerBlock = kThreads / kGroup;

struct Args {
    int64_t n_rows;      // n_envs * popcount(mask) selected rows
    const uint16_t* x;   // bf16 bits
    int64_t x_stride;
    uint16_t* act;       // [rows][6] int8 as three 2-B words
    uint32_t mask;
    int32_t n_agents, m;  // m = popcount(mask)
    // header columns, 16 bits each: hdr[0] = health, x, y, angle; hdr[1] = w,
    // team, zone x, zone y; hdr[2] = zone r, heal_slot_mask (unused: a valid column)
    uint64_t hdr[3];
    int32_t o_oth, o_othm, o_heal, o_healm;
    int32_t rec, off;    // an others record's width; health's index in it
    int32_t teams, n_others, n_cand;  // n_cand: others, then (FORAGER) heals
    Rule rule;
};

__device__ __forceinline__ float bf(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }

// The k-th (from 0) set bit of mask, k < popcount(mask) (as in mas_select.hip).
__device__ __forceinline__ int nth_set_bit(uint32_t mask, int k)
{
    int pos = 0;
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        const int c = __popc((mask >> pos) & ((1u << w) - 1u));
        const bool up = k >= c;
        pos = up ? pos + w : pos;
        k = up ? k - c : k;
    }
    return pos;
}

__device__ __forceinline__ Cand shfl_xor(Cand c, int d)
{
    Cand r;
    r.d2 = __shfl_xor(c.d2, d, kGroup);
    r.idx = __shfl_xor(c.idx, d, kGroup);
    r.x = __shfl_xor(c.x, d, kGroup);
    r.y = __shfl_xor(c.y, d, kGroup);
    return r;
}

__global__ __launch_bounds__(kThreads) void k_bot_act(const Args a)
{
    const int g = threadIdx.x & (kGroup - 1);
    const int64_t j0 = (int64_t)blockIdx.x * kRowsPerBlock;  // block-uniform 64-bit divide below
    if (j0 >= a.n_rows) return;
    const int64_t env0 = j0 / a.m;
    const uint32_t s = (uint32_t)(j0 - env0 * a.m) + (uint32_t)(threadIdx.x / kGroup);  // below m + 32
    const int64_t j = j0 + threadIdx.x / kGroup;
    const bool ok = j < a.n_rows;
    const uint32_t de = s / (uint32_t)a.m;
    int64_t row = (env0 + de) * a.n_agents + nth_set_bit(a.mask, (int)(s - de * (uint32_t)a.m));
    {
        // past the end: the last selected row again
        const int64_t last_env = (a.n_rows - 1) / a.m;
        const int64_t last = last_env * a.n_agents + nth_set_bit(a.mask, a.m - 1);
        row = ok ? row : last;
    }
    const uint16_t* __restrict__ xr = a.x + row * a.x_stride;

    // header fields g and 8 + (g & 1), broadcast over the group
    const uint32_t c0 = (uint32_t)(((g < 4 ? a.hdr[0] : a.hdr[1]) >> (16 * (g & 3))) & 0xffffu);
    const uint32_t c1 = (uint32_t)((a.hdr[2] >> (16 * (g & 1))) & 0xffffu);
    const float f0 = bf(xr[c0]), f1 = bf(xr[c1]);
    Self me;
    me.health = __shfl(f0, 0, kGroup);
    me.x = __shfl(f0, 1, kGroup);
    me.y = __shfl(f0, 2, kGroup);
    me.theta = __shfl(f0, 3, kGroup);
    me.w = __shfl(f0, 4, kGroup);
    const float team = __shfl(f0, 5, kGroup);
    me.zx = __shfl(f0, 6, kGroup);
    me.zy = __shfl(f0, 7, kGroup);
    me.zr = __shfl(f1, 0, kGroup);
    me.hsm = __shfl(f1, 1, kGroup);
    const float m2 = zone_m2(me.zr);

    Cand enemy = no_cand(), heal = no_cand();
    for (int q = g; q < a.n_cand; q += kGroup) {
        if (q < a.n_others) {
            const uint16_t* __restrict__ p = xr + a.o_oth + q * a.rec;
            const float msk = bf(xr[a.o_othm + q]);
            const float hp = bf(p[a.off]), ox = bf(p[a.off + 1]), oy = bf(p[a.off + 2]);
            const float ot = bf(p[a.teams ? 1 : 0]);
            Cand c;
            c.d2 = sq_dist(ox, oy, me.x, me.y);
            c.idx = q;
            c.x = ox;
            c.y = oy;
            if (msk == 0.0f && hp > 0.0f && !(a.teams && ot == team)) enemy = nearer(enemy, c);
        } else {
            const int k = q - a.n_others;
            const float msk = bf(xr[a.o_healm + k]);
            const float hx = bf(xr[a.o_heal + 2 * k]), hy = bf(xr[a.o_heal + 2 * k + 1]);
            Cand c;
            c.d2 = sq_dist(hx, hy, me.x, me.y);
            c.idx = k;
            c.x = hx;
            c.y = hy;
            if (msk == 0.0f && !(sq_dist(hx, hy, me.zx, me.zy) > m2)) heal = nearer(heal, c);
        }
    }
#pragma unroll
    for (int d = 1; d < kGroup; d <<= 1) {
        enemy = nearer(enemy, shfl_xor(enemy, d));
        heal = nearer(heal, shfl_xor(heal, d));
    }
    uint16_t w[3];
    decide(a.rule, me, heal, enemy, w);
    if (ok && g == 0) {
        uint16_t* q = a.act + row * 3;
        q[0] = w[0], q[1] = w[1], q[2] = w[2];
    }
}

}  // namespace bot

// Host side of mas_bot_act (arguments validated in mas_capi.hip, which also
// supplies the layout's columns): one launch, stream-ordered, no allocation.
int64_t bot_act_blocks(int64_t n_rows) { return (n_rows + bot::kRowsPerBlock - 1) / bot::kRowsPerBlock; }

hipError_t bot_act(int kind, int64_t n_envs, int n_agents, uint32_t mask, int teams, int n_heals, int o_agent,
                   int o_zone, int o_oth, int o_othm, int o_heal, int o_healm, int o_hsm, float use_below, float reach,
                   const void* x, int64_t x_stride, int8_t* actions, hipStream_t s)
{
    bot::Args a{};
    a.m = __builtin_popcount(mask);
    a.n_rows = n_envs * a.m;
    a.x = static_cast<const uint16_t*>(x);
    a.x_stride = x_stride;
    a.act = reinterpret_cast<uint16_t*>(actions);
    a.mask = mask;
    a.n_agents = n_agents;
    a.teams = teams ? 1 : 0;
    a.rec = 8 + a.teams;
    a.off = 1 + a.teams;
    const uint64_t ag = (uint64_t)o_agent, hp = ag + a.off;
    const uint64_t team = a.teams ? ag + 1 : ag, hsm = n_heals > 0 ? (uint64_t)o_hsm : (uint64_t)o_zone;
    a.hdr[0] = hp | (hp + 1) << 16 | (hp + 2) << 32 | (hp + 3) << 48;
    a.hdr[1] = (hp + 6) | team << 16 | (uint64_t)o_zone << 32 | (uint64_t)(o_zone + 1) << 48;
    a.hdr[2] = (uint64_t)(o_zone + 2) | hsm << 16;
    a.o_oth = o_oth;
    a.o_othm = o_othm;
    a.o_heal = o_heal;
    a.o_healm = o_healm;
    a.n_others = n_agents - 1;
    a.n_cand = a.n_others + (kind == bot::kForager ? n_heals : 0);
    a.rule.kind = kind;
    a.rule.n_heals = n_heals;
    a.rule.use_below = use_below;
    a.rule.reach = reach;
    const int64_t blocks = bot_act_blocks(a.n_rows);
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bot::k_bot_act, dim3((unsigned)blocks), dim3(bot::kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mas
