// mas_policy.h -- the host launchers of mas_policy.hip, as mas_capi.hip calls
// them.  Both units include this file, so a launcher whose definition drifts
// from its declaration fails to compile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mas {

int64_t policy_packed_bytes(int D);
int64_t policy_blocks(int64_t M);
hipError_t policy_pack(int D, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                       const float* b3, void* packed, hipStream_t s);
hipError_t policy_act(const void* packed, int D, int64_t M, const float* obs, void* xb, int64_t xb_stride,
                      uint64_t seed, uint64_t step, int64_t first_row, int8_t* act, float* logp, float* value,
                      hipStream_t s);
hipError_t policy_act_sel(const void* packed, int D, int64_t n_envs, int n_agents, uint32_t mask, const void* xb,
                          int64_t xb_stride, uint64_t seed, uint64_t step, int64_t first_row, bool greedy,
                          int8_t* act, float* logp, float* value, float* logits_out, hipStream_t s);

// One PPO train call, from the C ABI's arguments (include/masurvival.h
// mas_policy_train*) to the launch
enum class TrainForm {
    kStored,    // feature-major activations, all five stored (mas_policy_train, _ld, _w)
    kRowMajor,  // row-major activations (mas_policy_train_rm)
    kDw3,       // dW3 summed in the kernel, h2 and dz null and not stored (mas_policy_train_dw3, _dw3_w)
};
struct TrainCall {
    TrainForm form;
    bool weighted;  // the _w entry points: row_w required; else row_w is null
    const void* packed;
    int D;
    int64_t M;
    const void* xb;  // [M][xb_stride] bf16
    int64_t xb_stride;
    const int8_t* act;                          // [M][6]
    const float *old_logp, *adv, *ret, *row_w;  // [M]
    float clip, vf_coef, ent_coef, scale;
    void *h1, *h2, *da1, *da2, *dz;  // bf16
    int64_t ld;  // row stride of the feature-major buffers (>= M); kRowMajor: of h1 / h2 (ld_h)
    float *partials, *dw3_out, *scratch;  // dw3_out, scratch: kDw3 only, else null
};
// kDw3: only where policy_train_dw3_ok (mas_policy.hip)
bool policy_train_dw3_ok(int D, int64_t M, int64_t ld);
hipError_t policy_train(const TrainCall& c, hipStream_t s);

int policy_rm_feature(int col);
int64_t policy_adam_scratch();
hipError_t policy_adam(int64_t n, float* p, const float* g, float* m, float* v, float grad_scale, float max_norm,
                       double lr, double b1, double b2, double eps, int64_t step, float* scratch, hipStream_t s);
int64_t policy_dw_scratch(int F, int G, int64_t K);
hipError_t policy_dw(int F, int G, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, float* out,
                     float* scratch, hipStream_t s);

}  // namespace mas
