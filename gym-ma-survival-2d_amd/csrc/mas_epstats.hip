// mas_epstats.hip -- mas_episode_stats (include/masurvival.h): the episodes a
// rollout finished, their lengths, every agent slot's undiscounted return and
// which side won, from the rewards [T][E * A] and done flags [T][E] the
// rollout left in HBM, with a per-env carry across rollouts.
//
// One thread per env (not per agent column as k_ret_stats): the win rule needs
// all of an env's returns in one place at a done step, and envs do not tile a
// wave when A does not divide 64.  The kernel is a template on A = 1..kMaxAgents
// so the returns and their sums stay in named registers.  The rows of kChunk
// steps are loaded before the chunk's recurrence runs (as k_ret_stats and
// k_gae_walk prefetch, mas_capi.hip), so the serial walk waits on HBM once per
// chunk and not once per step.
//
// Reduction without atomics or library state: every workgroup stores its
// 6 + 2A partial sums into its own slots of the caller's scratch,
// scratch[v * nblocks + block], and a second launch of one workgroup adds the
// slots of every value in a fixed order (gae_block_part / k_gae_sums of
// mas_capi.hip, generalised from 2 values to NV).  Every slot read is written
// first, so the result does not depend on what the scratch held.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mas {
namespace eps {

// build-time choices (csrc/Makefile VFLAGS; measured in DESIGN.md 7.7)
#ifndef MAS_EP_WG
#define MAS_EP_WG 64
#endif
#ifndef MAS_EP_CHUNK
#define MAS_EP_CHUNK 8
#endif
constexpr int kWG = MAS_EP_WG;        // envs (threads) per workgroup
constexpr int kChunk = MAS_EP_CHUNK;  // steps whose rows are loaded ahead of the recurrence
constexpr int kMaxAgents = 8;         // the capacity classes' limit
constexpr int kSumThreads = 256;      // the one workgroup of k_ep_sums
static_assert(kWG % 64 == 0 && kWG >= 64 && kWG <= 1024, "whole waves");

constexpr int n_values(int A) { return 6 + 2 * A; }

// the workgroup's sums of v[0..NV) into part[v * nblocks + blockIdx.x]: wave
// butterflies (every lane ends with the wave's sum), then the waves in order
template <int NV>
__device__ __forceinline__ void block_part(double (&v)[NV], double* __restrict__ part, int nblocks)
{
#pragma unroll
    for (int i = 0; i < NV; ++i)
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
    if constexpr (kWG == 64) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) part[(int64_t)i * nblocks + blockIdx.x] = v[i];
        }
    } else {
        constexpr int kWaves = kWG / 64;
        __shared__ double ws[kWaves][NV];
        const int w = (int)(threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) ws[w][i] = v[i];
        }
        __syncthreads();
        if (threadIdx.x < NV) {
            double s = ws[0][threadIdx.x];
            for (int k = 1; k < kWaves; ++k) s += ws[k][threadIdx.x];
            part[(int64_t)threadIdx.x * nblocks + blockIdx.x] = s;
        }
    }
}

template <int A>
__global__ __launch_bounds__(kWG) void k_episode_stats(int T, int64_t E, uint32_t mask, const float* __restrict__ rew,
                                                       const uint8_t* __restrict__ done,
                                                       double* __restrict__ ret_carry, int32_t* __restrict__ len_carry,
                                                       double* __restrict__ part, int nblocks)
{
    constexpr int NV = n_values(A);
    const int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x;
    const bool sides = mask != 0u && mask != (1u << A) - 1u;  // two sides: wins and draws are counted
    double G[A], sg[A], sg2[A];
    double sl = 0.0, sl2 = 0.0;
    uint32_t episodes = 0, w0 = 0, w1 = 0, draws = 0;  // at most T each: exact
#pragma unroll
    for (int a = 0; a < A; ++a) sg[a] = sg2[a] = 0.0;
    if (e < E) {
        const int64_t M = E * A;
        const float* __restrict__ rp = rew + e * A;
        const uint8_t* __restrict__ dp = done + e;
        int32_t len = len_carry[e];
#pragma unroll
        for (int a = 0; a < A; ++a) G[a] = ret_carry[e * A + a];
        // one step: the rewards count, then the episode closes if the step is a done step
        auto step = [&](const float (&r)[A], uint8_t d) {
#pragma unroll
            for (int a = 0; a < A; ++a) G[a] += (double)r[a];
            len += 1;
            if (d) {
                const double L = (double)len;
                episodes += 1;
                sl += L;
                sl2 += L * L;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    sg[a] += G[a];
                    sg2[a] += G[a] * G[a];
                    if ((mask >> a) & 1u)
                        s0 += G[a];
                    else
                        s1 += G[a];
                    G[a] = 0.0;
                }
                if (sides) {
                    w0 += s0 > s1;
                    w1 += s1 > s0;
                    draws += s0 == s1;
                }
                len = 0;
            }
        };
        int t = 0;
        for (; t + kChunk <= T; t += kChunk) {
            float r[kChunk][A];
            uint8_t d[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const int64_t row = t + k;
#pragma unroll
                for (int a = 0; a < A; ++a) r[k][a] = rp[row * M + a];
                d[k] = dp[row * E];
            }
#pragma unroll
            for (int k = 0; k < kChunk; ++k) step(r[k], d[k]);
        }
        for (; t < T; ++t) {
            float r[A];
#pragma unroll
            for (int a = 0; a < A; ++a) r[a] = rp[(int64_t)t * M + a];
            step(r, dp[(int64_t)t * E]);
        }
        len_carry[e] = len;
#pragma unroll
        for (int a = 0; a < A; ++a) ret_carry[e * A + a] = G[a];
    }
    double v[NV];
    v[0] = (double)episodes, v[1] = sl, v[2] = sl2;
    v[3] = (double)w0, v[4] = (double)w1, v[5] = (double)draws;
#pragma unroll
    for (int a = 0; a < A; ++a) v[6 + a] = sg[a], v[6 + A + a] = sg2[a];
    block_part<NV>(v, part, nblocks);
}

// record[v] = the sum of value v's nblocks slots, fixed order: thread k adds
// slots k, k + 256, ..., then a butterfly and the four waves in order.  The NV
// loads of one slot index are independent, so a pass costs one round trip
template <int NV>
__global__ __launch_bounds__(kSumThreads) void k_ep_sums(const double* __restrict__ part, int nblocks,
                                                         double* __restrict__ record)
{
    const int k = (int)threadIdx.x;
    double s[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = 0.0;
    for (int b = k; b < nblocks; b += kSumThreads) {
#pragma unroll
        for (int i = 0; i < NV; ++i) s[i] += part[(int64_t)i * nblocks + b];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
        for (int off = 32; off > 0; off >>= 1) s[i] += __shfl_xor(s[i], off, 64);
    __shared__ double ws[kSumThreads / 64][NV];
    if ((k & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) ws[k >> 6][i] = s[i];
    }
    __syncthreads();
    if (k < NV) record[k] = ws[0][k] + ws[1][k] + ws[2][k] + ws[3][k];
}

template <int A>
void launch(int nblocks, int T, int64_t E, uint32_t mask, const float* rew, const uint8_t* done, double* ret_carry,
            int32_t* len_carry, double* record, double* scratch, hipStream_t s)
{
    hipLaunchKernelGGL(k_episode_stats<A>, dim3((unsigned)nblocks), dim3(kWG), 0, s, T, E, mask, rew, done, ret_carry,
                       len_carry, scratch, nblocks);
    hipLaunchKernelGGL(k_ep_sums<n_values(A)>, dim3(1), dim3(kSumThreads), 0, s, (const double*)scratch, nblocks,
                       record);
}

}  // namespace eps

int episode_stats_max_agents() { return eps::kMaxAgents; }

// workgroups of one call (envs / kWG, rounded up; no sum that could overflow)
int64_t episode_stats_blocks(int64_t n_envs) { return n_envs / eps::kWG + (n_envs % eps::kWG != 0); }

// Host side of mas_episode_stats (arguments validated in mas_capi.hip): two
// launches, stream-ordered, no allocation.
hipError_t episode_stats(int T, int64_t n_envs, int n_agents, uint32_t side_mask, const float* rewards,
                         const uint8_t* done, double* ret_carry, int32_t* len_carry, double* record, double* scratch,
                         hipStream_t s)
{
    const int nb = (int)episode_stats_blocks(n_envs);
#define MAS_EP_CASE(A)                                                                                      \
    case A:                                                                                                 \
        eps::launch<A>(nb, T, n_envs, side_mask, rewards, done, ret_carry, len_carry, record, scratch, s); \
        break;
    switch (n_agents) {
        MAS_EP_CASE(1)
        MAS_EP_CASE(2)
        MAS_EP_CASE(3)
        MAS_EP_CASE(4)
        MAS_EP_CASE(5)
        MAS_EP_CASE(6)
        MAS_EP_CASE(7)
        MAS_EP_CASE(8)
    default:
        return hipErrorInvalidValue;
    }
#undef MAS_EP_CASE
    return hipGetLastError();
}

}  // namespace mas
