// Shared pieces of the rollout kernel family (K10+K11):
//   rollout.hip     v6, the general kernel, and the one dispatcher
//   rollout_v7.hip  v7, MFMA kernel for the linear policy at the Humanoid geometry
//   rollout_m7.hip  m7, MLP-64 kernel at the Humanoid geometry
// Helpers only one kernel uses stay with that kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "check.h"

namespace ea {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

__device__ __forceinline__ __bf16 f2b(float v) { return (__bf16)v; }
__device__ __forceinline__ float b2f(__bf16 v) { return (float)v; }

// tanh via the hardware exp unit (v_exp_f32): ~1e-6 relative error —
// far below the bf16 quantization (2^-8) every value passes through;
// libm tanhf is branchy code on the hot path.
__device__ __forceinline__ float tanh_fast(float x) {
    const float xc = fminf(fmaxf(x, -15.0f), 15.0f);
    // e^(2x) = 2^(x · 2·log2(e)) with the doubling folded into the constant
    // (0x4038aa3b, exactly twice the log2(e) that __expf multiplies by):
    // one multiply feeds v_exp_f32, and the product rounds to the same bits
    // as __expf(2.0f * xc) since 2·xc is exact
    const float e = __builtin_amdgcn_exp2f(xc * __builtin_bit_cast(float, 0x4038aa3bu));
    // v_rcp_f32 (~1 ulp) instead of an IEEE divide: the result is bf16-
    // quantized immediately, so the 2^-23-level rcp error is invisible
    return (e - 1.0f) * __builtin_amdgcn_rcpf(e + 1.0f);
}

// Lane sums on the VALU pipe via DPP modifiers — __shfl_down lowers to
// ds_bpermute_b32 on the LDS pipe, where it fights the dot-product LDS
// reads (v7's policy phase measured 85 such ops per lane per step).
template <int kCtrl>
__device__ __forceinline__ float dpp_add(float x) {
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), kCtrl, 0xf, 0xf, true);
    return x + __builtin_bit_cast(float, moved);
}

// x + (y moved across lanes by DPP control kCtrl)
template <int kCtrl>
__device__ __forceinline__ float dpp_add_from(float x, float y) {
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), kCtrl, 0xf, 0xf, true);
    return x + __builtin_bit_cast(float, moved);
}

// 8-lane group sum: valid in the TOP lane of each 8-lane group
__device__ __forceinline__ float group8_sum_dpp(float x) {
    x = dpp_add<0x111>(x);  // row_shr:1
    x = dpp_add<0x112>(x);  // row_shr:2
    x = dpp_add<0x114>(x);  // row_shr:4
    return x;
}

// 32-lane sum: after row_shr 1/2/4/8 + row_bcast:15 the totals sit in
// lanes 31 and 63
__device__ __forceinline__ float reduce32_dpp(float x) {
    x = dpp_add<0x111>(x);  // row_shr:1
    x = dpp_add<0x112>(x);  // row_shr:2
    x = dpp_add<0x114>(x);  // row_shr:4
    x = dpp_add<0x118>(x);  // row_shr:8
    x = dpp_add<0x142>(x);  // row_bcast:15
    return x;
}

struct RolloutArgs {
    const float* params;      // [n_members][L]
    const float* env_blob;    // packed fp32 env data (see EnvBlob)
    float* fitness_out;       // [n_members]
    float* obs_stats_out;     // [rows][2][O] (sum, sumsq) partials: one row per block (v7, m7) or per
                              // (block, member) (v6), plain stores; the dispatcher sums the rows
    int n_members;
    long member_offset;       // global id of member 0 (rank sharding)
    int obs_dim, act_dim, rank, steps;
    float alive_bonus, act_cost;
    unsigned long long init_seed;
    const unsigned long long* seed_ptr;  // device episode seed (hipGraph-safe); overrides init_seed
    int hidden;               // policy hidden width, 0 = linear policy
    // early termination (the kTerm instantiations of v6 and v7; the other kernels ignore these):
    // a member is done after the step whose bf16(o'[health_index]) leaves
    // [healthy_lo, healthy_hi] (NaN counts as outside)
    int health_index;
    float healthy_lo, healthy_hi;
    int* steps_out;           // [n_members] episode lengths
};

// env_blob layout (fp32, SyntheticEnvSpec.env_blob): V [R][O] · U_T [R][O] ·
// D2_T [A][O] · c [O] · wr [O] · mean [O] · std [O]. U_T and D2_T are
// adjacent, so U_T also addresses the R + A rows of [U;D2].
struct EnvBlob {
    const float *V, *U_T, *D2_T, *c, *wr, *mean, *std;
    __device__ __forceinline__ EnvBlob(const float* blob, int O, int A, int R)
        : V(blob), U_T(V + (long)R * O), D2_T(U_T + (long)R * O), c(D2_T + (long)A * O), wr(c + O), mean(wr + O),
          std(mean + O) {}
};

constexpr int kV7MembersPerBlock = 16;
constexpr int kM7MembersPerBlock = 2;

// Launch entry points of rollout_v7.hip and rollout_m7.hip (Humanoid
// geometry only; args.obs_stats_out holds one row per block). v7 with
// `terminating` runs its early-termination instantiation, which reads the
// health fields of args and writes args.steps_out.
void launch_rollout_v7(const RolloutArgs& args, int n, hipStream_t stream, bool terminating);
void launch_rollout_m7(const RolloutArgs& args, int n, hipStream_t stream);

}  // namespace ea
