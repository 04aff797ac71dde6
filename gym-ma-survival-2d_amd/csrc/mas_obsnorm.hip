// mas_obsnorm.hip -- running observation normalisation (include/masurvival.h
// mas_obs_stats, mas_obs_norm_merge, mas_policy_pack_norm).  The normaliser
// never touches a row: it is folded into the packed layer-1 weights,
//   W1 ((x - mu) * s) + b1 = (W1 diag(s)) x + (b1 - W1 (mu * s)),
// so the act and train kernels (mas_policy.hip) run unchanged on raw rows.
//
// k_obs_stats   per-column sum and sum of squares of bf16 rows, in fp64.  One
//               lane per (row of the pass, 16-B chunk of the row): a tile of W
//               chunks (W = the row's ceil(n_cols / 8) chunks, at most 256 at a
//               time) by R = 256 / W rows.  A workgroup owns a contiguous
//               range of rows and walks it R rows per pass, so a pass reads R
//               row segments of W * 16 B that lie one row stride apart (at the
//               policy's strides a row is 18, 22 or 60 chunks of which 18, 20,
//               59 are read: nearly one contiguous range).  kU passes of loads
//               are issued before the first is used.  Each lane keeps 8 + 8
//               fp64 accumulators (bf16 -> double and x * x are exact); after
//               the walk the R rows of the tile are summed through LDS in row
//               order and the workgroup stores one partial record
//               [2][8 * chunks] into the caller's scratch.
// k_obs_finish  the records summed per output: 32 threads each add a contiguous
//               share of the records in block order, one adds the 32 parts.
//               The grid of both depends on (n_rows, n_cols) alone and every
//               sum has a fixed order: same inputs, same bits.  No atomics.
// k_obs_merge   Chan's merge of (count_b, sum, sum of squares) into the
//               running (count, mean, m2), one workgroup, a thread per column;
//               every thread reads the count before the barrier, one writes it
//               after.
// k_fold        the layer-1 fragments and bias of a packed image written again
//               with the normaliser folded in (after policy_pack wrote the
//               whole image): fragment element bf16(W1[f][k] * s[k]), bias
//               b1[f] - sum_k w1r[f][k] * mu[k] in fp64 over ascending k from
//               the ROUNDED weights w1r -- the MFMA multiplies x by those, so a
//               column that sits at its mean cancels only against them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mas_policy.h"

namespace mas {
namespace obsnorm {

constexpr int kThreads = 256;
constexpr int kU = 4;            // passes of loads in flight per lane
constexpr int kMaxBlocks = 1536; // 6 workgroups on each of 256 CUs: 6 waves per SIMD, all resident (72 VGPRs fit 7)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Plan {
    int cn;          // 16-B chunks of a row that hold a column below n_cols
    int64_t rpb;     // rows per workgroup
    int64_t blocks;  // workgroups (0: no rows)
    int64_t rec;     // doubles per partial record: 2 * 8 * cn
};

// a function of (n_rows, n_cols) alone
inline Plan make_plan(int64_t n_rows, int n_cols)
{
    Plan p{};
    p.cn = (n_cols + 7) / 8;
    p.rec = 16 * (int64_t)p.cn;
    if (n_rows <= 0) return p;
    const int w = p.cn < kThreads ? p.cn : kThreads;
    const int64_t r = kThreads / w;  // rows of one pass
    // at least kU passes per workgroup before the grid grows, then the cap
    int64_t blocks = (n_rows + r * kU - 1) / (r * kU);
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    p.rpb = (n_rows + blocks - 1) / blocks;
    p.rpb = (p.rpb + r - 1) / r * r;  // whole passes
    p.blocks = (n_rows + p.rpb - 1) / p.rpb;
    return p;
}

__device__ __forceinline__ void accumulate(const u32x4 v, double (&s)[8], double (&q)[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t w = v[j];
        const double lo = (double)__uint_as_float(w << 16);
        const double hi = (double)__uint_as_float(w & 0xffff0000u);
        s[2 * j] += lo;
        q[2 * j] = __builtin_fma(lo, lo, q[2 * j]);  // lo * lo is exact: the fused form rounds the same once
        s[2 * j + 1] += hi;
        q[2 * j + 1] = __builtin_fma(hi, hi, q[2 * j + 1]);
    }
}

__global__ __launch_bounds__(kThreads) void k_obs_stats(int64_t n_rows, int cn, int64_t rpb,
                                                        const uint16_t* __restrict__ x, int64_t x_stride,
                                                        double* __restrict__ scratch)
{
    __shared__ double lds[8 * kThreads];  // [accumulator][lane]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * rpb;
    const int64_t row1 = row0 + rpb < n_rows ? row0 + rpb : n_rows;
    double* rec = scratch + (int64_t)blockIdx.x * 16 * cn;
    for (int c0 = 0; c0 < cn; c0 += kThreads) {  // one tile unless a row has more than 256 chunks
        const int w = cn - c0 < kThreads ? cn - c0 : kThreads;
        const int r = kThreads / w;
        const int rr = tid / w, c = tid - rr * w;
        const bool lane_on = rr < r;
        double s[8] = {}, q[8] = {};
        if (lane_on) {
            const uint16_t* p = x + 8 * (int64_t)(c0 + c);
            int64_t row = row0 + rr;
            // kU passes at a time while all of them are inside the range
            for (; row + (int64_t)(kU - 1) * r < row1; row += (int64_t)kU * r) {
                u32x4 v[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u)
                    v[u] = *reinterpret_cast<const u32x4*>(p + (row + (int64_t)u * r) * x_stride);
#pragma unroll
                for (int u = 0; u < kU; ++u) accumulate(v[u], s, q);
            }
            for (; row < row1; row += r) accumulate(*reinterpret_cast<const u32x4*>(p + row * x_stride), s, q);
        }
        // the sums, then the squares, through the same 16 KiB
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            __syncthreads();  // the readers before are done with lds
#pragma unroll
            for (int k = 0; k < 8; ++k) lds[k * kThreads + tid] = kind == 0 ? s[k] : q[k];
            __syncthreads();
            // record element (kind, column 8 (c0 + cc) + k): the tile's rows in order
            for (int o = tid; o < 8 * w; o += kThreads) {
                const int k = o / w, cc = o - k * w;
                double a = lds[k * kThreads + cc];
                for (int i = 1; i < r; ++i) a += lds[k * kThreads + i * w + cc];
                rec[(int64_t)kind * 8 * cn + 8 * (c0 + cc) + k] = a;
            }
        }
    }
}

// kFinOut outputs per workgroup, each summed by kFinParts threads: part p adds
// its contiguous share of the records in block order, then one thread adds the
// parts in order (one thread per output walked all 1536 records alone: 0.5 ms).
constexpr int kFinOut = 8, kFinParts = kThreads / kFinOut;

__global__ __launch_bounds__(kThreads) void k_obs_finish(int n_cols, int cn, int64_t blocks,
                                                         const double* __restrict__ scratch,
                                                         double* __restrict__ sums)
{
    __shared__ double part[kFinParts][kFinOut];
    const int oo = threadIdx.x % kFinOut, pp = threadIdx.x / kFinOut;
    const int o = blockIdx.x * kFinOut + oo;
    const bool on = o < 2 * n_cols;
    double a = 0.0;
    if (on) {
        const int kind = o / n_cols, col = o - kind * n_cols;
        const double* p = scratch + (int64_t)kind * 8 * cn + col;
        const int64_t per = (blocks + kFinParts - 1) / kFinParts;
        const int64_t b1 = (pp + 1) * per < blocks ? (pp + 1) * per : blocks;
        for (int64_t b = pp * per; b < b1; ++b) a += p[b * 16 * cn];
    }
    part[pp][oo] = a;
    __syncthreads();
    if (pp == 0 && on) {
        double t = part[0][oo];
        for (int i = 1; i < kFinParts; ++i) t += part[i][oo];
        sums[o] = t;
    }
}

__global__ __launch_bounds__(kThreads) void k_obs_merge(int n_cols, double* __restrict__ state,
                                                        const double* __restrict__ batch, double eps,
                                                        float* __restrict__ mean_out, float* __restrict__ inv_std_out)
{
    const double count = state[0];
    const double nb = batch[0];
    const double n = count + nb;
    for (int c = threadIdx.x; c < n_cols; c += kThreads) {
        double mean = state[1 + c], m2 = state[1 + n_cols + c];
        if (nb > 0.0) {
            const double mean_b = batch[1 + c] / nb;
            const double m2_b = fmax(batch[1 + n_cols + c] - nb * mean_b * mean_b, 0.0);
            const double d = mean_b - mean;
            mean += d * nb / n;
            m2 += m2_b + d * d * count * nb / n;
            state[1 + c] = mean;
            state[1 + n_cols + c] = m2;
        }
        mean_out[c] = n > 0.0 ? (float)mean : 0.0f;
        inv_std_out[c] = n > 0.0 ? (float)(1.0 / sqrt(m2 / n + eps)) : 1.0f;
    }
    __syncthreads();  // every thread holds the old count
    if (threadIdx.x == 0 && nb > 0.0) state[0] = n;
}

// Where policy_pack (mas_policy.hip k_pack) puts layer 1 in the packed image:
// the fragments first, element t of them = (k-step ks, M-tile mt, lane l,
// element j) with t = ((ks * 8 + mt) * 64 + l) * 8 + j, holding W1[32 mt +
// (l & 31)][16 ks + 8 (l >> 5) + j]; the 256 pre-scaled biases b1p [8][2][16]
// 528 floats before the image's end, entry (mt, h, i) = feature 32 mt + (i &
// 3) + 8 (i >> 2) + 4 h.  The fold test (tests/test_gpu_pack_norm.py) holds
// this against policy_pack bit for bit.
constexpr float kTanhC = 2.8853900817779268f;  // 2 log2(e), as mas_policy.hip scales b1

__global__ __launch_bounds__(kThreads) void k_fold(int D, int ks1, int64_t b1_off, const float* __restrict__ W1,
                                                   const float* __restrict__ b1, const float* __restrict__ mean,
                                                   const float* __restrict__ inv_std, uint8_t* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nel = (int64_t)ks1 * 8 * 64 * 8;
    if (t < nel) {
        const int j = (int)(t & 7), l = (int)((t >> 3) & 63);
        const int64_t g = t >> 9;
        const int ks = (int)(g >> 3), mt = (int)(g & 7);
        const int k = 16 * ks + 8 * (l >> 5) + j;
        const float v = k < D ? W1[(int64_t)(32 * mt + (l & 31)) * D + k] * inv_std[k] : 0.0f;
        reinterpret_cast<__bf16*>(out)[t] = (__bf16)v;
        return;
    }
    const int rem = (int)(t - nel);
    if (rem >= 256) return;
    const int mt = rem / 32, h = (rem / 16) & 1, i = rem & 15;
    const int f = 32 * mt + (i & 3) + 8 * (i >> 2) + 4 * h;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < D; ++k) {
        const float w1r = (float)(__bf16)(W1[(int64_t)f * D + k] * inv_std[k]);
        acc += (double)w1r * (double)mean[k];  // an exact product: 8 x 24 bits
    }
    reinterpret_cast<float*>(out)[b1_off + rem] = (float)((double)b1[f] - acc) * kTanhC;
}

}  // namespace obsnorm

int64_t obs_stats_scratch_doubles(int64_t n_rows, int n_cols)
{
    const obsnorm::Plan p = obsnorm::make_plan(n_rows, n_cols);
    return p.blocks * p.rec;
}

// Host sides (arguments validated in mas_capi.hip): stream-ordered launches,
// no allocation, no synchronisation.
hipError_t obs_stats(int64_t n_rows, int n_cols, const void* x, int64_t x_stride, double* sums, double* scratch,
                     hipStream_t s)
{
    const obsnorm::Plan p = obsnorm::make_plan(n_rows, n_cols);
    if (p.blocks == 0) return hipMemsetAsync(sums, 0, sizeof(double) * 2 * (size_t)n_cols, s);
    hipLaunchKernelGGL(obsnorm::k_obs_stats, dim3((unsigned)p.blocks), dim3(obsnorm::kThreads), 0, s, n_rows, p.cn,
                       p.rpb, static_cast<const uint16_t*>(x), x_stride, scratch);
    hipLaunchKernelGGL(obsnorm::k_obs_finish, dim3((unsigned)((2 * n_cols + obsnorm::kFinOut - 1) / obsnorm::kFinOut)),
                       dim3(obsnorm::kThreads), 0, s, n_cols, p.cn, p.blocks, scratch, sums);
    return hipGetLastError();
}

hipError_t obs_norm_merge(int n_cols, double* state, const double* batch, double eps, float* mean_out,
                          float* inv_std_out, hipStream_t s)
{
    hipLaunchKernelGGL(obsnorm::k_obs_merge, dim3(1), dim3(obsnorm::kThreads), 0, s, n_cols, state, batch, eps,
                       mean_out, inv_std_out);
    return hipGetLastError();
}

hipError_t policy_pack_norm(int D, const float* W1, const float* b1, const float* W2, const float* b2,
                            const float* W3, const float* b3, const float* mean, const float* inv_std, void* packed,
                            hipStream_t s)
{
    const hipError_t e = policy_pack(D, W1, b1, W2, b2, W3, b3, packed, s);
    if (e != hipSuccess || !mean) return e;
    const int ks1 = (D + 15) / 16;
    const int64_t b1_off = policy_packed_bytes(D) / 4 - 16 - 2 * 256;  // floats: b1p, b2p, b3 end the image
    const int64_t n = (int64_t)ks1 * 8 * 64 * 8 + 256;
    hipLaunchKernelGGL(obsnorm::k_fold, dim3((unsigned)((n + obsnorm::kThreads - 1) / obsnorm::kThreads)),
                       dim3(obsnorm::kThreads), 0, s, D, ks1, b1_off, W1, b1, mean, inv_std, (uint8_t*)packed);
    return hipGetLastError();
}

}  // namespace mas
