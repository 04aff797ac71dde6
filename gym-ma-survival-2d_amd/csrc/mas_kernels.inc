// mas_kernels.inc -- MI355X (gfx950) kernels of the batched MaSurvival step,
// included once per capacity class (mas_k_<class>.hip) so that the classes
// compile in parallel.  64-lane workgroups (one wave), env state
// struct-of-arrays in HBM.  mas_step is the launch sequence (launch_step
// below):
//   k_pre_lanes     (env, agent) lanes: the pre_step rules and the speculative
//                   contact-free 2 x world.Step; the envs that leave the fast
//                   path go onto the sharded general-path list (mas_lanes.h)
//   k_gen_solve_g   a lane group per listed env: both world steps of the
//                   general path -- Collide, island Solve, SolveTOI -- in one
//                   launch (mas_gensolve.h)
//   k_post_lanes    (env, agent) lanes: every post-physics phase, rewards,
//                   done, stats, the auto-reset of the done envs in place and
//                   the obs rows (mas_post_lanes.h)
//   [k_lidar]       the Lidars columns, when configured
// and with the slow split a side stream runs the slow list's k_gen_solve_g
// and list-mode k_post_lanes.  k_obs / k_reset serve mas_reset and the
// auto-reset of configs whose spawn permutation does not fit k_post_lanes'
// LDS.
// Build flags (Makefile): -O3 -ffp-contract=off, IEEE f32 div/sqrt (hipcc
// default), -mllvm -pragma-unroll-threshold so every per-body loop unrolls and
// the env state stays in registers.
#pragma once
#include <hip/hip_runtime.h>

#include "mas_lanes.h"

namespace mas {

// ------------------------------------------------------------------------
// state load / store (mas_env.h state_index): one 4-B word per lane per
// access, a wave's access one coalesced 256-B row of the SoA image
// ------------------------------------------------------------------------
struct Loader {
    const uint32_t* __restrict__ base;
    int64_t N, e;
    int w;
    bool on = true;
    template <class T>
    __device__ void io(T& x)
    {
        if (on) {
            uint32_t u = base[state_index(w, e, N)];
            __builtin_memcpy(&x, &u, 4);
        }
        ++w;
    }
    template <class T>
    __device__ void io64(T& x)
    {
        uint32_t lo = 0, hi = 0;
        io(lo);
        io(hi);
        if (on) x = ((uint64_t)hi << 32) | lo;
    }
    __device__ void align4() { w = (w + 3) & ~3; }
    __device__ void cont(int n) { w += n; }
};

struct Storer {
    uint32_t* __restrict__ base;
    int64_t N, e;
    int w;
    bool on = true;
    template <class T>
    __device__ void io(T& x)
    {
        uint32_t u;
        __builtin_memcpy(&u, &x, 4);
        if (on) base[state_index(w, e, N)] = u;
        ++w;
    }
    template <class T>
    __device__ void io64(T& x)
    {
        uint32_t lo = (uint32_t)(x & 0xffffffffULL), hi = (uint32_t)(x >> 32);
        io(lo);
        io(hi);
    }
    __device__ void align4() { w = (w + 3) & ~3; }
    __device__ void cont(int n) { w += n; }
};

struct Finder {
    const void* target;
    int w = 0, found = -1, cont_at = -1;
    bool on = true;
    void align4() { w = (w + 3) & ~3; }
    void cont(int n)
    {
        cont_at = w;
        w += n;
    }
    template <class T>
    void io(T& x)
    {
        if ((const void*)&x == target) found = w;
        ++w;
    }
    template <class T>
    void io64(T& x)
    {
        if ((const void*)&x == target) found = w;
        w += 2;
    }
};

// ------------------------------------------------------------------------
// The reset and obs kernels of mas_reset (and of the auto-reset fallback,
// launch_post): k_reset resets masked envs one lane per env; k_obs (with the
// reset in front when a workgroup holds whole envs) writes obs rows one lane
// per (env, agent), staged in LDS and written back as contiguous row
// segments.  Each loads the state groups it reads and stores the ones it
// writes.
// ------------------------------------------------------------------------
constexpr uint32_t kResetLd = kGRng;
constexpr uint32_t kResetSt = kGAll & ~kGStat;
constexpr uint32_t kObsLd = kGDyn | kGRule | kGBox | kGItem | kGHeal | kGZone | kGSeen;

#define MAS_KERNEL __global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(1, 1)))
// kernels with several lanes per env (more waves than SIMDs): two waves per
// SIMD, so one wave's VALU and memory stalls are covered by the other's issue
#define MAS_KERNEL2 __global__ __launch_bounds__(kWG, 2)
// exactly `occ` waves per SIMD as the register budget (512 / occ VGPRs),
// class-dependent: the big classes' env state spills at 256 registers
#define MAS_KERNEL_OCC(occ) __global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(occ, occ)))

// The auto-reset runs inside k_obs for blocks holding a done env (k_obs
// comment) when a block holds whole envs (A == C::AM); otherwise k_reset
template <class C>
constexpr bool kObsReset = true;

// Entry p of the general-path list (or of a one-shard list): its shards are
// concatenated in shard order.  k0: the workgroup's first entry (any: the
// list reaches it), p: this lane's entry.  Every lane of the wave calls it
// (lane q < list_shards loads shard q's count; a wave prefix sum and one
// ballot per distinct entry of the wave locate the shards).
struct ListPos {
    bool any, valid;
    int64_t e;
};
__device__ __forceinline__ ListPos list_pos(const Params& P, int64_t N, int64_t k0, int64_t p)
{
    ListPos r;
    if (P.list_shards <= 1) {
        const int64_t cnt = min((int64_t)*P.phys_count, N);
        r.any = k0 < cnt;
        r.valid = p < cnt;
        r.e = r.valid ? (int64_t)P.phys_list[p] : 0;
        return r;
    }
    const int lane = (int)(threadIdx.x & 63);
    // (each shard's count clamped to its capacity, as the one-shard path
    // clamps to N: a count past its cap would index the next shard's entries)
    const int c = lane < P.list_shards ? min(P.phys_count[lane * kShardStride], P.list_cap) : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    const int64_t total = __shfl(incl, 63, 64);
    const int excl = incl - c;
    r.any = k0 < total;
    r.valid = p < total;
    // this lane's shard: the last shard whose first entry is <= p (p is one
    // of the wave's few distinct entries: one ballot per distinct value)
    int sh = 0, base = 0;
    int64_t q = p;
    while (true) {
        const int64_t pq = __shfl(q, __ffsll((unsigned long long)__ballot(q >= 0)) - 1, 64);
        const uint64_t le = __ballot(lane < P.list_shards && (int64_t)excl <= pq);
        const int shq = 63 - __clzll(le);
        const int bq = __shfl(excl, shq, 64);
        if (q == pq) {
            sh = shq;
            base = bq;
            q = -1;
        }
        if (!__any(q >= 0)) break;
    }
    r.e = r.valid ? (int64_t)P.phys_list[(int64_t)sh * P.list_cap + (p - base)] : 0;
    return r;
}

// The general path: one k_gen_solve_g launch for both world steps (Collide,
// island Solve, SolveTOI on a lane group per env over the compacted list,
// mas_gensolve.h).  Waves per SIMD (the register budget): 2.
template <class C>
constexpr int kSolveOcc = 2;
// Both world steps through one copy of the world step's code (a rolled loop)
// in the classes with up to 4 agent slots: half the kernel's code (2v2:
// 234 KB -> 111 KB), fewer SGPR spills (229 -> 109) and no scratch.  The 8-slot
// classes (xl, xxl), which spill either way, take more scratch in the loop
// form (232 -> 236 and 200 -> 228 B per lane) and keep the two inlined copies.
template <class C>
constexpr bool kSolveRolled = C::AM <= 4;
template <class C>
MAS_KERNEL_OCC(kSolveOcc<C>) void k_gen_solve_g(Params P, uint32_t* __restrict__ state, int64_t N, int ws)
{
    using SS = SolveShape<C>;
    __shared__ float rec[kRecW * SS::KL * SS::EPW];
    __shared__ uint32_t toi_snap[kToiSnapW * SS::EPW];  // the previous TOI event per group (toi_agent_group)
    const int slot = (int)threadIdx.x / SS::G, s = (int)threadIdx.x % SS::G;
    // (the main list in XCD-aware runs of 16 waves: a shard's entries, one
    // contiguous env range of k_pre, mostly on one XCD)
    const int64_t gb = P.gen_sparse ? (int64_t)blockIdx.x : xcd_block_run<16>();
    const ListPos lp = list_pos(P, N, P.gen_sparse ? gb : gb * SS::EPW,
                                P.gen_sparse ? (int64_t)slot * gridDim.x + gb : gb * SS::EPW + slot);
    if (!lp.any) return;  // the whole workgroup (one wave)
    MAS_PROF(P, -1);
    const bool valid = lp.valid;
    // ws = -1: both world steps in this launch.  The second reloads what the
    // first stored, by other lanes of this wave: a workgroup-scope fence (the
    // wave is the workgroup) orders those stores before its loads
    if constexpr (kSolveRolled<C>) {
        // Every iteration takes the kernel arguments, the state base and the
        // env index from behind an opaque point: what the body derives from
        // them (the Params fields, the env's state addresses) would otherwise
        // be hoisted out of the loop and held in registers across the whole
        // world step, which spilled (2v2: 576 B of scratch per lane).
        const int nws = ws < 0 ? 2 : 1;
#pragma nounroll
        for (int k = 0; k < nws; ++k) {
            if (k) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                MAS_PROF(P, 7);  // the fence's wait for the first world step's stores
            }
            KernParams kpar = KernParams::get();
            kpar.reread();
            const int64_t e = (int64_t)opq((uint64_t)lp.e);
            gen_solve_group<C>(*kpar, opq_s(state), opq_s(N), e, valid, s, rec, toi_snap, slot, 8 * k);  // (phases 0.. / 8..)
        }
    } else {
        const int64_t e = lp.e;
        gen_solve_group<C>(P, state, N, e, valid, s, rec, toi_snap, slot, 0);
        if (ws < 0) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            MAS_PROF(P, 7);  // the fence's wait for the first world step's stores
            gen_solve_group<C>(P, state, N, e, valid, s, rec, toi_snap, slot, 8);
        }
    }
    MAS_PROF_FLUSH(P, P.gen_sparse ? 4 : 0, 0);
}

// Env selection of the post-physics kernels (k_post_lanes, k_obs).
// kAllEnvs: every env, one stream.  The slow split (launch_step)
// runs kMainEnvs on the caller's stream (every env but the slow list's,
// gen_flag 2) and kGenEnvs over the slow list on the handle's side stream;
// envs are independent, so the two selections touch disjoint state,
// rewards, done flags and obs rows.
enum : int { kAllEnvs = 0, kGenEnvs = 2, kMainEnvs = 3 };
template <int M>
__device__ __forceinline__ int64_t gen_list_count(const Params& P, int64_t N)
{
    return M == kGenEnvs ? min((int64_t)*P.phys_count, N) : N;
}
// env e belongs to the other stream's selection
template <int M>
__device__ __forceinline__ bool other_stream(const Params& P, int64_t e)
{
    return M == kMainEnvs ? P.gen_flag[e] == 2 : false;
}
// The general-path list's only readers are the general kernels, which run
// before the first post kernel on the caller's stream: that kernel (kAllEnvs
// or kMainEnvs) keeps the count for mas_debug_counters and zeroes it for the
// next step on the device, so a captured and replayed step starts its list
// empty like an eager one.  (The side stream's selection reads its own list,
// the slow list.)
template <int M>
__device__ __forceinline__ void retire_phys_count(const Params& P)
{
    if (M == kGenEnvs || blockIdx.x != 0) return;
    // (every shard: lane q takes shard q's count; the workgroup is one wave)
    const int lane = (int)(threadIdx.x & 63);
    const bool mine = lane < kListShards;  // (every shard: list_shards may differ between steps)
    int c = mine ? P.phys_count[lane * kShardStride] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o, 64);
    if (mine) P.phys_count[lane * kShardStride] = 0;
    if (lane == 0) *P.phys_last = c;
}

template <class C>
struct ResetLds {
    float tab[FixTab<C>::kWords * kWG];
    uint16_t pairs[Scr<C>::kPairs * kWG];
    uint32_t seen[C::NB * kWG];
    uint8_t perm[256 * kWG];
};

// BaseEnv.reset of the masked envs, one lane per env (mas_reset, and the
// auto-reset when k_obs cannot take it: A < C::AM)
template <class C>
MAS_KERNEL void k_reset(Params P, uint32_t* __restrict__ state, int64_t N, const uint8_t* __restrict__ mask)
{
    __shared__ ResetLds<C> lds;
    const int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (e >= N) return;
    if (mask && !mask[e]) return;
    EnvL<C> L;
    Loader ld{state, N, e, 0};
    visit_state(L, ld, kResetLd);
    Scr<C> scr{lds.pairs, lds.seen, lds.perm, (int)threadIdx.x};
    env_reset(L, P, scr);
    FixTab<C> T{lds.tab, (int)threadIdx.x};
    build_fixtab(L, P, T);
    update_seen(L, P, scr, T);
    seen_pack(L, scr);
#pragma unroll
    for (int k = 0; k < Cont<C>::kWords; ++k) state[state_index(P.w_cont + k, e, N)] = 0u;
    P.slow_flag[e] = 0;  // a new episode: no slow-list history
    Storer st{state, N, e, 0};
    visit_state(L, st, kResetSt);
}

// k_obs column window: rows are built kObsW columns at a time into an LDS
// tile [64 rows][kObsW+1] (odd stride: conflict-free row writes), and each
// tile row goes out as one coalesced 256-B store per wave.
constexpr int kObsW = 64;

struct WinRow {
    float* p;
    int c0;
    __device__ void operator()(int k, float v)
    {
        // out-of-window writes land in the padding column: no branch
        const unsigned kk = (unsigned)(k - c0);
        p[kk < (unsigned)kObsW ? kk : (unsigned)kObsW] = v;
    }
    // does [off, off+len) meet the window (wave-uniform)
    __device__ bool want(int off, int len) const { return off < c0 + kObsW && off + len > c0; }
};

// k_obs with the reset in front (auto-reset, launch_step / launch_reset when
// A == C::AM divides kWG, so a workgroup's rows are whole envs): lane j < kWG / A of the
// workgroup resets the block's env j when reset_mask[e] (BaseEnv.reset:
// env_reset, Cameras.post_reset, contact memory cleared, every group but the
// stats stored), then the block writes the obs rows.  Only blocks holding a
// done env pay the reset; the others go straight to the obs (the separate
// k_reset launch made every step pay the longest reset before any obs row).
// The reset scratch is per env of the block and shares the LDS of the obs
// tile.
template <class C>
constexpr int kObsResetCols = kWG / C::AM;  // reset scratch columns: the block's envs when A == C::AM
template <class C>
constexpr int kObsResetBytes = (int)(sizeof(float) * FixTab<C, kObsResetCols<C>>::kWords * kObsResetCols<C> +
                                     sizeof(uint16_t) * Scr<C, kObsResetCols<C>>::kPairs * kObsResetCols<C> +
                                     sizeof(uint32_t) * C::NB * kObsResetCols<C> + 256 * kObsResetCols<C>);
template <class C>
constexpr int kObsLdsFloats = (int)(kWG * (kObsW + 1)) > (kObsResetBytes<C> + 3) / 4 ? (int)(kWG * (kObsW + 1))
                                                                                    : (kObsResetBytes<C> + 3) / 4;

// k_obs waves per SIMD: 2 for the small classes; the ffa / xl rows (BM = 16 /
// 8) spilled ~1.6 KB per lane at 256 registers (FFA x16384: k_obs 378 ->
// 153 us per step with the whole register file; the launch is one wave per
// SIMD anyway)
template <class C>
constexpr int kObsOcc = C::BM > 4 ? 1 : 2;
// kGenEnvs (the split step's general envs): block b holds the listed envs
// k0 = b * (kWG / A) .. k0 + kWG / A - 1, row j * A + i of the tile is agent i
// of listed env j, and the tile rows go out to their scattered obs rows.
template <class C, bool R, int M>
MAS_KERNEL_OCC(kObsOcc<C>) void k_obs(Params P, uint32_t* __restrict__ state, int64_t N, const uint8_t* __restrict__ mask,
                      float* __restrict__ obs, const uint8_t* __restrict__ reset_mask)
{
    // the obs tile, and before it (same bytes) the reset scratch of the
    // block's envs: [k][S] columns, S = kWG / A envs per block (A == C::AM)
    __shared__ float tile[kObsLdsFloats<C>];
    const int A = P.A, D = P.D;
    const int64_t rows = N * A;
    const int64_t r0 = (int64_t)blockIdx.x * kWG;
    const int epb = kWG / A;
    const int64_t cnt = gen_list_count<M>(P, N);
    const int64_t k0 = (int64_t)blockIdx.x * epb;  // kGenEnvs: the block's first listed env
    if (M == kGenEnvs && k0 >= cnt) return;        // the whole workgroup (one wave)
    MAS_PROF(P, -1);
    if (R && reset_mask) {
        // every row of this block belongs to env r0 / A + j, j < kWG / A
        // (kGenEnvs: listed env k0 + j)
        const int64_t eb = r0 / A;
        const int j = (int)threadIdx.x;
        bool mine;
        int64_t ej;
        if (M == kGenEnvs) {
            mine = j < epb && k0 + j < cnt;
            ej = mine ? (int64_t)P.phys_list[k0 + j] : 0;
        } else {
            ej = eb + j;
            mine = j < epb && ej < N && !other_stream<M>(P, ej);
        }
        mine = mine && reset_mask[ej];
        if (__any(mine)) {
            constexpr int S = kObsResetCols<C>;
            float* tab = tile;
            uint16_t* pairs = reinterpret_cast<uint16_t*>(tab + FixTab<C, S>::kWords * S);
            uint32_t* seen = reinterpret_cast<uint32_t*>(pairs + Scr<C, S>::kPairs * S);
            uint8_t* perm = reinterpret_cast<uint8_t*>(seen + C::NB * S);
            // (a lane that is not a reset lane keeps an empty env: it only
            // joins the dealt camera rays)
            const int jc = mine ? j : 0;
            const int64_t e = mine ? ej : eb;
            EnvL<C> L;
            Scr<C, S> scr{pairs, seen, perm, jc};
            FixTab<C, S> T{tab, jc};
            if (mine) {
                Loader ld{state, N, e, 0};
                visit_state(L, ld, kResetLd);
                env_reset(L, P, scr);
                build_fixtab(L, P, T);
            }
            // Cameras.post_reset: the camera rays of the block's reset envs,
            // dealt over its lanes (the pair list area is the ray list)
            update_seen_dealt(L, P, scr, T, mine, pairs);
            if (mine) {
                seen_pack(L, scr);
#pragma unroll
                for (int k = 0; k < Cont<C>::kWords; ++k) state[state_index(P.w_cont + k, e, N)] = 0u;
                P.slow_flag[e] = 0;  // a new episode: no slow-list history
                Storer st{state, N, e, 0};
                visit_state(L, st, kResetSt);
            }
            __syncthreads();  // the reset envs' state is stored (workgroup scope) and the scratch is free
        }
    }
    MAS_PROF(P, 37);
    int64_t r, e;
    int i;
    bool active;
    if (M == kGenEnvs) {
        const int j = (int)threadIdx.x / A;
        i = (int)threadIdx.x - j * A;
        active = j < epb && k0 + j < cnt;
        e = active ? (int64_t)P.phys_list[k0 + j] : 0;
        r = e * A + i;
        active = active && (!mask || mask[e]);
    } else {
        r = r0 + threadIdx.x;
        e = r / A;
        i = (int)(r - e * A);
        active = r < rows && (!mask || mask[e]) && !other_stream<M>(P, e);
    }
    const uint64_t act = __ballot(active);
    EnvL<C> L;
    if (active) {
        Loader ld{state, N, e, 0};
        visit_state(L, ld, kObsLd);
    }
    MAS_PROF(P, 38);
    float* row_tile = tile + threadIdx.x * (kObsW + 1);
    for (int c0 = 0; c0 < D; c0 += kObsW) {
        if (active) {
            WinRow sink{row_tile, c0};
            write_obs_row(L, P, i, sink);
        }
        wave_lds_sync();  // the tile's rows are in LDS (one-wave block; no wait for the stores)
        MAS_PROF(P, 39);
        if (M == kGenEnvs) {
            // scattered rows: tile row q goes to obs row r of lane q
            const int rr = (int)r;  // N * A < 2^31 (mas_create)
#pragma unroll
            for (int cc = 0; cc < kObsW; cc += kWG) {
                const int col = c0 + cc + (int)threadIdx.x;
                const bool col_ok = cc + (int)threadIdx.x < kObsW && col < D;
                const float* src = tile + cc + threadIdx.x;
                for (int q0 = 0; q0 < kWG; q0 += 16) {
                    float v[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[k] = col_ok ? src[(q0 + k) * (kObsW + 1)] : 0.0f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int rq = __shfl(rr, q0 + k, 64);
                        if (col_ok && ((act >> (q0 + k)) & 1ull)) obs[(int64_t)rq * D + col] = v[k];
                    }
                }
            }
        } else
#pragma unroll
        for (int cc = 0; cc < kObsW; cc += kWG) {
            // lane = column cc + lane of the window
            const bool col_ok = cc + (int)threadIdx.x < kObsW && c0 + cc + (int)threadIdx.x < D;
            float* dst = obs + r0 * D + c0 + cc + threadIdx.x;
            const float* src = tile + cc + threadIdx.x;
            if (act == ~0ull) {
                // every row of the block is active (the common case): no
                // per-row tests
                for (int q0 = 0; q0 < kWG; q0 += 16) {
                    float v[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[k] = col_ok ? src[(q0 + k) * (kObsW + 1)] : 0.0f;
                    if (col_ok) {
#pragma unroll
                        for (int k = 0; k < 16; ++k) dst[(int64_t)k * D] = v[k];
                    }
                    dst += (int64_t)16 * D;
                }
            } else {
                for (int q0 = 0; q0 < kWG; q0 += 16) {
                    float v[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[k] = col_ok ? src[(q0 + k) * (kObsW + 1)] : 0.0f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        if (col_ok && ((act >> (q0 + k)) & 1ull)) *dst = v[k];
                        dst += D;
                    }
                }
            }
        }
        wave_lds_sync();  // the tile's reads are done before the next window's rows
        MAS_PROF(P, 40);
    }
    // (over a list -- the fused auto-reset fallback, which may run on both
    // streams of the slow split at once -- its own kid, ADVICE r05)
    MAS_PROF_FLUSH(P, M == kGenEnvs ? 6 : 3, 37);
}

// Lidars (opt-in 'lidars' key): one lane per (env, agent, laser) ray, after
// k_obs, writing the key's columns of the obs rows of the active envs
constexpr uint32_t kLidLd = kGDyn | kGBox | kGItem | kGHeal;
template <class C>
MAS_KERNEL2 void k_lidar(Params P, const uint32_t* __restrict__ state, int64_t N, const uint8_t* __restrict__ mask,
                         float* __restrict__ obs)
{
    const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
    const int64_t r = t / P.n_lasers;  // (env, agent) row
    const int k = (int)(t - r * P.n_lasers);
    const int64_t e = r / P.A;
    if (e >= N || (mask && !mask[e])) return;
    EnvL<C> L;
    Loader ld{const_cast<uint32_t*>(state), N, e, 0};
    visit_state(L, ld, kLidLd);
    obs[r * P.D + P.o_lid + k] = lidar_depth(L, P, (int)(r - e * P.A), k);
}

template <class C>
void launch_lidar(hipStream_t s, const Params& P, const uint32_t* st, int64_t N, const uint8_t* m, float* ob)
{
    if (P.n_lasers <= 0) return;
    const dim3 gl((unsigned)((N * P.A * P.n_lasers + kWG - 1) / kWG));
    hipLaunchKernelGGL(k_lidar<C>, gl, dim3(kWG), 0, s, P, st, N, m, ob);
}

// host launchers, explicitly instantiated once per capacity class (one TU each)
struct ClassInfo {
    int words, w_rng, w_has32, w_stats, w_cont, w_invdt, lds_bytes;
    int am, post_union;  // agent slots; k_post_lanes' LDS union bytes (the in-place reset's permutation scratch)
    int w_alive;         // state word of the alive mask (StateWords<C>::alive)
};

template <class C>
ClassInfo class_info()
{
    ClassInfo o;
    EnvL<C>* L = new EnvL<C>();
    Finder f;
    f.target = &L->st_hi;
    visit_state(*L, f);
    o.words = f.w;
    o.w_rng = f.found;
    Finder f2;
    f2.target = &L->has32;
    visit_state(*L, f2);
    o.w_has32 = f2.found;
    Finder f3;
    f3.target = &L->stats[0];
    visit_state(*L, f3);
    o.w_stats = f3.found;
    o.w_cont = f3.cont_at;
    Finder f4;
    f4.target = &L->inv_dt0;
    visit_state(*L, f4);
    o.w_invdt = f4.found;
    // StateWords (the kernels' compile-time word indices) against the visit order
    {
        using TW = StateWords<C>;
        const void* t[5] = {&L->alive_m, &L->awake_m, &L->nbox, &L->bp[C::BM - 1].x, &L->bmeta[C::BM - 1]};
        const int want[5] = {TW::alive, TW::awake, TW::box, TW::box + 1 + 6 * (C::BM - 1), TW::box + 5 + 6 * (C::BM - 1)};
        for (int k = 0; k < 5; ++k) {
            Finder fk;
            fk.target = t[k];
            visit_state(*L, fk);
            if (fk.found != want[k]) o.words = -1;  // mas_create refuses the class
        }
    }
    // Lay (mas_lanes.h: the agent-lane kernels' group offsets) against the visit order
    {
        using LY = Lay<C>;
        Finder fc;
        fc.target = nullptr;
        visit_state(*L, fc);
        const void* t[10] = {&L->health[0], &L->nbox, &L->nbi, &L->npend, &L->nheal, &L->zc[0].x, &L->inv_dt0,
                             &L->st_hi, &L->stats[0], &L->seenw[0]};
        const int want[10] = {LY::rule, LY::box, LY::item, LY::pend, LY::heal, LY::zone, LY::invdt, LY::rng, LY::stat,
                              LY::seen};
        for (int k = 0; k < 10; ++k) {
            Finder fk;
            fk.target = t[k];
            visit_state(*L, fk);
            if (fk.found != want[k]) o.words = -1;  // mas_create refuses the class
        }
        if (fc.cont_at != LY::cont) o.words = -1;
    }
    delete L;
    o.w_alive = StateWords<C>::alive;  // (checked against the visit order above)
    o.lds_bytes = (int)sizeof(ResetLds<C>);
    return o;
}

}  // namespace mas
#include "mas_post_lanes.h"  // (uses the env selections, Loader / Storer and retire_phys_count above)
namespace mas {

// the post-physics phases over one env selection (M), on stream s
template <class C, int M>
void launch_post(dim3 g, hipStream_t s, const Params& P, uint32_t* st, int64_t N, float* ob, float* rw, uint8_t* dn,
                 bool fuse, bool reset_sep)
{
    const bool ar = fuse || reset_sep || P.reset_in_post;
    const dim3 gp((unsigned)((N + kWG / C::AM - 1) / (kWG / C::AM)));
    hipLaunchKernelGGL((k_post_lanes<C, M>), gp, dim3(kWG), 0, s, P, st, N, ob, rw, dn, ar ? 1 : 0);
    if (!ar || P.reset_in_post) return;  // (reset_in_post: k_post_lanes reset its done envs)
    // the auto-reset of this selection's done envs (k_post_lanes' list):
    // k_obs over the list resets them and writes their rows (A == C::AM),
    // else k_reset (masked by done) and k_obs over the list
    Params R = P;
    R.phys_list = P.reset_list;
    R.phys_count = P.reset_count;
    R.list_shards = 1;
    R.gen_sparse = 0;
    const dim3 go((unsigned)((N * P.A + kWG - 1) / kWG));
    if (fuse) {
        hipLaunchKernelGGL((k_obs<C, true, kGenEnvs>), go, dim3(kWG), 0, s, R, st, N, (const uint8_t*)nullptr, ob,
                           (const uint8_t*)dn);
    } else {
        hipLaunchKernelGGL(k_reset<C>, g, dim3(kWG), 0, s, P, st, N, (const uint8_t*)dn);
        hipLaunchKernelGGL((k_obs<C, false, kGenEnvs>), go, dim3(kWG), 0, s, R, st, N, (const uint8_t*)nullptr, ob,
                           (const uint8_t*)nullptr);
    }
}

// the general physics path of the envs k_pre flagged, on stream s: one
// k_gen_solve_g for both world steps (MAS_GEN_FUSE2=0: one per world step)
template <class C>
void launch_general(hipStream_t s, const Params& P, uint32_t* st, int64_t N)
{
    const dim3 gs((unsigned)((N + SolveShape<C>::EPW - 1) / SolveShape<C>::EPW));
    // both world steps in one launch (a wave's envs run their second world
    // step as soon as their first is done, instead of after the whole first
    // launch's slowest wave); MAS_GEN_FUSE2=0 (read once): one launch per
    // world step.  Measured (r04r, env-only 2v2 x65536, two processes each):
    // 0.324 / 0.330 vs 0.339 / 0.342 ms/step
    static const bool fuse2 = [] {
        const char* v = getenv("MAS_GEN_FUSE2");
        return !(v && v[0] == '0');
    }();
    if (fuse2) {
        hipLaunchKernelGGL((k_gen_solve_g<C>), gs, dim3(kWG), 0, s, P, st, N, -1);
        return;
    }
    for (int k = 0; k < 2; ++k) hipLaunchKernelGGL((k_gen_solve_g<C>), gs, dim3(kWG), 0, s, P, st, N, k);
}

// mas_step.  The slow split (sp non-null): after k_pre the side stream runs
// the slow list's general path and post phases (one env per wave: a few
// envs' long SolveTOI chains) while the caller's stream runs the general
// path over the main list and the post phases of every other env; the
// caller's stream then waits for the side stream (and runs the Lidars over
// every env).  Same state, rewards, done flags and obs as the one-stream
// order: the envs are independent.
template <class C>
void launch_step(dim3 g, hipStream_t s, const Params& P0, uint32_t* st, int64_t N, const int8_t* a, float* ob,
                 float* rw, uint8_t* dn, int ar, const StepSplit* sp)
{
    // the auto-reset: inside k_post_lanes when the spawn permutation fits its
    // LDS (reset_in_post), else a reset launch over each post kernel's done
    // list (k_obs with the reset in front when A == C::AM, else k_reset + k_obs)
    const bool rip = ar && reset_fits_post<C>(P0);
    const bool fuse = ar && !rip && kObsReset<C> && P0.A == C::AM && (kWG % P0.A) == 0;
    const bool split = sp && (!ar || fuse || rip);
    // the slow list exists only in the slow split (elsewhere nothing would run it)
    Params P = P0;
    P.slow_route = split ? 1 : 0;
    P.reset_in_post = rip ? 1 : 0;
    // the general-path list's shards: each takes the appends of at most
    // ceil(blocks / shards) k_pre blocks (a contiguous run in the XCD-aware
    // order, mas_lanes.h), so at most their envs
    {
        const int64_t nblk = (N + kWG / C::AM - 1) / (kWG / C::AM);
        const int64_t cap = (nblk + kListShards - 1) / kListShards * (kWG / C::AM);
        const bool sharded = cap * kListShards <= N + kListSlack;
        P.list_shards = sharded ? kListShards : 1;
        P.list_cap = sharded ? (int)cap : (int)N;
    }
    const dim3 gpl((unsigned)((N + kWG / C::AM - 1) / (kWG / C::AM)));
    hipLaunchKernelGGL(k_pre_lanes<C>, gpl, dim3(kWG), 0, s, P, st, N, a);
    if (split) {
        (void)hipEventRecord(sp->fork, s);
        (void)hipStreamWaitEvent(sp->side, sp->fork, 0);
        Params Q = P;
        Q.phys_list = P.slow_list;
        Q.phys_count = P.slow_count;
        Q.list_shards = 1;
        Q.gen_sparse = 1;
        Q.reset_list = P.reset_list + N;  // the side stream's own auto-reset list (without the reset in place)
        Q.reset_count = P.reset_count + 1;
        launch_general<C>(sp->side, Q, st, N);
        launch_post<C, kGenEnvs>(g, sp->side, Q, st, N, ob, rw, dn, fuse, false);
        launch_general<C>(s, P, st, N);
        launch_post<C, kMainEnvs>(g, s, P, st, N, ob, rw, dn, fuse, false);
        (void)hipEventRecord(sp->join, sp->side);
        (void)hipStreamWaitEvent(s, sp->join, 0);
    } else {
        launch_general<C>(s, P, st, N);
        launch_post<C, kAllEnvs>(g, s, P, st, N, ob, rw, dn, fuse, ar && !fuse && !rip);
    }
    launch_lidar<C>(s, P, st, N, nullptr, ob);
}

// Render view of one env (debugging / frames, not on the step path): one
// thread loads env e's bodies and writes the float layout of
// mas_render_view (include/masurvival.h) from word kViewHead on; the host
// fills the header and walls.
constexpr int kViewHead = 32;
template <class C>
__global__ void k_view(Params P, const uint32_t* __restrict__ state, int64_t N, int64_t e, float* __restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    EnvL<C> L;
    Loader ld{const_cast<uint32_t*>(state), N, e, 0};
    visit_state(L, ld, kGDyn | kGRule | kGBox | kGItem | kGHeal | kGZone);
    out[0] = (float)P.A;
    out[1] = (float)L.nbox;
    out[2] = (float)L.nbi;
    out[3] = (float)L.nheal;
    out[4] = L.zpos.x;
    out[5] = L.zpos.y;
    out[6] = L.zrad;
    out[7] = (float)C::AM;
    out[8] = (float)C::BM;
    out[9] = (float)C::HM;
    float* o = out + kViewHead;
    for (int i = 0; i < C::AM; ++i, o += 5) {
        o[0] = L.c[i].x;
        o[1] = L.c[i].y;
        o[2] = L.a[i];
        o[3] = bit(L.alive_m, i) ? 1.0f : 0.0f;
        o[4] = (float)L.health[i];
    }
    for (int b = 0; b < C::BM; ++b, o += 5) {
        o[0] = L.bp[b].x;
        o[1] = L.bp[b].y;
        o[2] = L.bhx[b];
        o[3] = L.bhy[b];
        o[4] = (float)L.bhealth[b];
    }
    for (int b = 0; b < C::BM; ++b, o += 4) {
        o[0] = L.ip[b].x;
        o[1] = L.ip[b].y;
        o[2] = L.ihx[b];
        o[3] = L.ihy[b];
    }
    for (int k = 0; k < C::HM; ++k, o += 2) {
        o[0] = L.hp[k].x;
        o[1] = L.hp[k].y;
    }
}

template <class C>
void launch_view(hipStream_t s, const Params& P, const uint32_t* st, int64_t N, int64_t e, float* out)
{
    hipLaunchKernelGGL(k_view<C>, dim3(1), dim3(64), 0, s, P, st, N, e, out);
}

template <class C>
void launch_reset(dim3 g, hipStream_t s, const Params& P, uint32_t* st, int64_t N, const uint8_t* m, float* ob)
{
    const dim3 go((unsigned)((N * P.A + kWG - 1) / kWG));
    const bool fuse = ob && m && kObsReset<C> && P.A == C::AM && (kWG % P.A) == 0;
    if (!fuse) hipLaunchKernelGGL(k_reset<C>, g, dim3(kWG), 0, s, P, st, N, m);
    if (ob) {
        if (fuse)
            hipLaunchKernelGGL((k_obs<C, true, kAllEnvs>), go, dim3(kWG), 0, s, P, st, N, m, ob, m);
        else
            hipLaunchKernelGGL((k_obs<C, false, kAllEnvs>), go, dim3(kWG), 0, s, P, st, N, m, ob, (const uint8_t*)nullptr);
        launch_lidar<C>(s, P, st, N, m, ob);
    }
}

}  // namespace mas

#define MAS_INSTANTIATE(NAME, CAPT)                                                                          \
    namespace mas {                                                                                         \
    ClassInfo class_info_##NAME()                                                                           \
    {                                                                                                       \
        ClassInfo o = class_info<CAPT>();                                                                   \
        o.am = CAPT::AM;                                                                                    \
        o.post_union = kPostUnionBytes<CAPT>;                                                               \
        return o;                                                                                           \
    }                                                                                                       \
    void launch_step_##NAME(dim3 g, hipStream_t s, const Params& P, uint32_t* st, int64_t N, const int8_t* a, \
                            float* ob, float* rw, uint8_t* dn, int ar, const StepSplit* sp)                 \
    {                                                                                                       \
        launch_step<CAPT>(g, s, P, st, N, a, ob, rw, dn, ar, sp);                                           \
    }                                                                                                       \
    void launch_reset_##NAME(dim3 g, hipStream_t s, const Params& P, uint32_t* st, int64_t N, const uint8_t* m, \
                             float* ob)                                                                     \
    {                                                                                                       \
        launch_reset<CAPT>(g, s, P, st, N, m, ob);                                                          \
    }                                                                                                       \
    void launch_view_##NAME(hipStream_t s, const Params& P, const uint32_t* st, int64_t N, int64_t e, float* o) \
    {                                                                                                       \
        launch_view<CAPT>(s, P, st, N, e, o);                                                               \
    }                                                                                                       \
    }
