// mas_select.hip -- mas_rows_select (include/masurvival.h): gather the rows of
// the bit-selected agents of whole envs into dense arrays.  The self-play
// trainer compacts the learner's share of a rollout with it once per
// iteration, so GAE, the advantage normalisation and the train / weight-
// gradient kernels run unchanged on dense rows.  A pure copy: no LDS, no
// scratch, every offset 64-bit.
//
// Logical (output) row j of n_envs * m rows, m = popcount(mask), is physical
// (input) row (j / m) * n_agents + (the (j % m)-th set bit of the mask) -- the
// remap of k_policy_act_sel (mas_policy.hip).  Rows of unselected agents are
// never read; nothing past output row n_envs * m is written.
//
// One launch, two block ranges (block-uniform branch):
//   x      bf16 rows as 16-B chunks, cpr = x_cols / 8 per row.  The chunks of
//          all output rows form one sequence c = j * cpr + k; consecutive lanes
//          take consecutive c, so a wave-instruction stores 1 KiB of contiguous
//          output and loads whole contiguous runs (a run ends where a row's
//          x_cols end or the next selected agent is not the next physical
//          row).  A row is no power-of-two number of chunks (18, 22, 60 at the
//          classes' strides), so c is split by division: a wave divides its
//          first chunk once (64-bit, wave-uniform: row, then env), each lane
//          divides only its small offset from there: a multiply by a
//          reciprocal the host made (Div).  kU chunks per lane, every load
//          issued before the first store.
//   rows   one lane per logical row: its 6 action bytes (three 2-B words) and
//          up to kMaxF32 fp32 scalars, same wave-uniform env divide.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mas {
namespace sel {

constexpr int kThreads = 256;
constexpr int kU = 4;        // 16-B chunks per lane of the x range
constexpr int kMaxF32 = 4;   // fp32 arrays of one call (include/masurvival.h)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// n / d for the small n the lanes divide (offsets from the wave's first row:
// n < d + 64 * kU): one 32 x 33-bit multiply by mul = ceil(2^32 / d), exact
// while n * (mul * d - 2^32) < 2^32, which n < d + 256 and d <= 32768 give;
// a larger d (mul == 0, big) has n < 2 * d, so the quotient is a compare.
// Branch-free: one of the two terms is zero.
struct Div {
    uint32_t d, big;
    uint64_t mul;
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const
    {
        return (uint32_t)(((uint64_t)n * mul) >> 32) + (big & (uint32_t)(n >= d));
    }
};
inline Div make_div(uint32_t d)
{
    const bool big = d > 32768u;
    return Div{d, big ? 1u : 0u, big ? 0ull : ((1ull << 32) + d - 1) / d};
}

struct Args {
    int64_t n_rows;     // n_envs * m logical rows
    int64_t n_chunks;   // n_rows * cpr (0: no x pair)
    int64_t x_blocks;   // blocks [0, x_blocks) copy x, the rest the per-row arrays
    int32_t n_agents;
    uint32_t mask;
    Div m, cpr;         // selected agents per env; 16-B chunks per x row
    const uint16_t* x;  // bf16 bits
    uint16_t* x_out;
    int64_t x_stride, x_out_stride;
    const uint16_t* act;  // [rows][6] int8 as three 2-B words
    uint16_t* act_out;
    int32_t n_f32;
    const float* f_in[kMaxF32];
    float* f_out[kMaxF32];
};

// The k-th (from 0) set bit of mask, k < popcount(mask): five branch-free
// halvings on the popcount of the lower half of what is left (as in
// mas_policy.hip, whose translation unit this one does not share code with).
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

__global__ __launch_bounds__(kThreads) void k_rows_select(const Args a)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t m = a.m.d;
    if ((int64_t)blockIdx.x < a.x_blocks) {
        const uint32_t cpr = a.cpr.d;
        const int64_t c0 = wave * (64 * kU);  // the wave's first chunk
        if (c0 >= a.n_chunks) return;
        // wave-uniform: logical row of c0 and its chunk there, then env and agent slot
        const int64_t j0 = c0 / cpr;
        const uint32_t k0 = (uint32_t)(c0 - j0 * cpr);
        const int64_t env0 = j0 / m;
        const uint32_t s0 = (uint32_t)(j0 - env0 * m);
        // a lane past the last chunk loads the last chunk again (an address
        // that is always valid: the loads need no branch) and stores nothing
        const uint32_t last = (uint32_t)(a.n_chunks - c0 - 1 < 64 * kU - 1 ? a.n_chunks - c0 - 1 : 64 * kU - 1);
        u32x4 v[kU];
        uint32_t dj[kU], k[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t o = (uint32_t)(64 * u + lane);
            // offsets from (j0, chunk 0): below cpr + 64 * kU
            const uint32_t d = k0 + (o < last ? o : last);
            dj[u] = a.cpr(d);
            k[u] = d - dj[u] * cpr;
            const uint32_t s = s0 + dj[u];  // agent slots from (env0, slot 0): below m + 64 * kU
            const uint32_t de = a.m(s);
            const int64_t row = (env0 + de) * a.n_agents + nth_set_bit(a.mask, (int)(s - de * m));
            v[u] = *reinterpret_cast<const u32x4*>(a.x + row * a.x_stride + 8 * (int64_t)k[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if ((uint32_t)(64 * u + lane) <= last)
                *reinterpret_cast<u32x4*>(a.x_out + (j0 + dj[u]) * a.x_out_stride + 8 * (int64_t)k[u]) = v[u];
        return;
    }
    const int64_t j0 = (wave - a.x_blocks * (kThreads / 64)) * 64;
    if (j0 >= a.n_rows) return;
    const int64_t j = j0 + lane;
    const bool ok = j < a.n_rows;
    const int64_t env0 = j0 / m;  // wave-uniform 64-bit divide; the lane's offset is below 64 + m
    const uint32_t s = (uint32_t)((ok ? j : a.n_rows - 1) - env0 * m);  // past the end: the last row again
    const uint32_t de = a.m(s);
    const int64_t row = (env0 + de) * a.n_agents + nth_set_bit(a.mask, (int)(s - de * m));
    // every load before the first store
    uint16_t w0 = 0, w1 = 0, w2 = 0;
    float fv[kMaxF32] = {};
    if (a.act) {
        const uint16_t* p = a.act + row * 3;
        w0 = p[0], w1 = p[1], w2 = p[2];
    }
#pragma unroll
    for (int f = 0; f < kMaxF32; ++f)
        if (f < a.n_f32) fv[f] = a.f_in[f][row];
    if (!ok) return;
    if (a.act) {
        uint16_t* q = a.act_out + j * 3;
        q[0] = w0, q[1] = w1, q[2] = w2;
    }
#pragma unroll
    for (int f = 0; f < kMaxF32; ++f)
        if (f < a.n_f32) a.f_out[f][j] = fv[f];
}

}  // namespace sel

// Host side of mas_rows_select (arguments validated in mas_capi.hip; NULL
// pairs skipped): one launch, stream-ordered, no allocation.
hipError_t rows_select(int64_t n_envs, int n_agents, uint32_t mask, const void* x, int64_t x_stride, void* x_out,
                       int64_t x_out_stride, int x_cols, const int8_t* act, int8_t* act_out, int n_f32,
                       const float* const* f_in, float* const* f_out, hipStream_t s)
{
    sel::Args a{};
    const int m = __builtin_popcount(mask);
    a.m = sel::make_div((uint32_t)m);
    a.n_rows = n_envs * m;
    a.n_agents = n_agents;
    a.mask = mask;
    a.cpr = sel::make_div(x ? (uint32_t)(x_cols / 8) : 1u);
    a.n_chunks = x ? a.n_rows * a.cpr.d : 0;
    a.x = static_cast<const uint16_t*>(x);
    a.x_out = static_cast<uint16_t*>(x_out);
    a.x_stride = x_stride;
    a.x_out_stride = x_out_stride;
    a.act = reinterpret_cast<const uint16_t*>(act);
    a.act_out = reinterpret_cast<uint16_t*>(act_out);
    for (int f = 0; f < n_f32; ++f)
        if (f_in[f]) {
            a.f_in[a.n_f32] = f_in[f];
            a.f_out[a.n_f32] = f_out[f];
            ++a.n_f32;
        }
    constexpr int64_t kChunksPerBlock = (int64_t)sel::kThreads * sel::kU;
    a.x_blocks = (a.n_chunks + kChunksPerBlock - 1) / kChunksPerBlock;
    const int64_t r_blocks = (act || a.n_f32 > 0) ? (a.n_rows + sel::kThreads - 1) / sel::kThreads : 0;
    const int64_t blocks = a.x_blocks + r_blocks;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(sel::k_rows_select, dim3((unsigned)blocks), dim3(sel::kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mas
