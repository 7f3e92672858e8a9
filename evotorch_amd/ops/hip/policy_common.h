// What the population-batched stack forwards share: K13
// (policy_forward.hip, every member on its own observation), K14
// (policy_forward_shared.hip, every member on one shared minibatch, fp32
// MFMA), K15 (policy_forward_shared_bf16.hip, the same on bf16 MFMA) and K16
// (policy_forward_recurrent.hip, K13 with one RNN or LSTM layer in the stack).
#pragma once
#include <hip/hip_runtime.h>
#include <c10/util/Exception.h>

#include <cstdint>
#include <vector>

#include "reduce.h"
#include "rollout_common.h"

namespace ea {

constexpr int kMaxLayers = 4;
constexpr int kMaxWidth = 1024;
enum PolicyActivation : int { kActIdentity = 0, kActTanh = 1, kActRelu = 2 };

typedef float floatx4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float policy_activation(float v, int act) {
    if (act == kActTanh) return tanhf(v);             // the accurate one, not tanh_fast
    if (act == kActRelu) return v < 0.0f ? 0.0f : v;  // NaN passes, as torch.relu passes it
    return v;
}

// K13 and K16: the per-member GEMV layer, its group sum and the fence between layers.

// Sum over each group of G lanes, valid in the group's LAST lane.
template <int G>
__device__ __forceinline__ float group_sum(float x) {
    if constexpr (G == 8) {
        return group8_sum_dpp(x);
    } else {
        x = dpp_add<0x111>(x);  // row_shr:1
        x = dpp_add<0x112>(x);  // row_shr:2
        x = dpp_add<0x114>(x);  // row_shr:4
        x = dpp_add<0x118>(x);  // row_shr:8: lane 15 of each 16-lane row
        if constexpr (G == 64) {
            // rows 0..3 in lane order: ((r0 + r1) + r2) + r3, read on the scalar pipe
            const int xi = __builtin_bit_cast(int, x);
            const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 15));
            const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 31));
            const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 47));
            x = ((r0 + r1) + r2) + x;  // lane 63 holds r3
        }
        return x;
    }
}

// Orders this wave's LDS stores before its later LDS loads (other lanes' data).
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One layer of one member: y[0:N) = act(W [N][K] · x[0:K) + b). x is in LDS;
// y is LDS or global. Runs with all 64 lanes active.
template <int G>
__device__ __forceinline__ void policy_layer(const float* __restrict__ W, const float* __restrict__ b,
                                             const float* x, float* y, int K, int N, int act, int lane) {
    constexpr int kRowsPerPass = kWaveSize / G;
    const int gl = lane & (G - 1);
    const int group = lane / G;
    const int words = K >> 2;                 // whole 16-byte words of a row
    const int steps = (words + G - 1) / G;    // wave-uniform trip count
    const int tail = K & 3;
    const floatx4* x4 = reinterpret_cast<const floatx4*>(x);
    for (int row0 = 0; row0 < N; row0 += kRowsPerPass) {
        const int row = row0 + group;
        const float* Wr = W + (long)min(row, N - 1) * K;
        float acc = 0.0f;
#pragma unroll 4
        for (int s = 0; s < steps; ++s) {
            const int w = gl + s * G;
            const bool in = w < words;
            const int wc = in ? w : 0;  // words >= 1 here, so word 0 is inside the row
            const floatx4_a4 wv = *reinterpret_cast<const floatx4_a4*>(Wr + 4 * wc);
            const floatx4 xv = x4[wc];
            float t = fmaf(wv.x, xv.x, acc);
            t = fmaf(wv.y, xv.y, t);
            t = fmaf(wv.z, xv.z, t);
            t = fmaf(wv.w, xv.w, t);
            acc = in ? t : acc;
        }
        if (gl < tail) {  // G >= 8 > 3: one trailing element per lane
            const int k = 4 * words + gl;
            acc = fmaf(Wr[k], x[k], acc);
        }
        acc = group_sum<G>(acc);
        if (gl == G - 1 && row < N) {
            if (b != nullptr) acc += b[row];
            y[row] = policy_activation(acc, act);
        }
    }
}

// Lanes per row group of a layer with K inputs: the narrowest group whose
// lanes make at most 2 (G = 8) or 8 (G = 16) steps along the row. K = 3
// leaves 7 of 8 lanes idle instead of 63 of 64; K = 376 (94 words) runs
// 6 steps on four rows at once; only K > 512 spreads a row over the wave.
inline int policy_group_width(int K) {
    const int words = K / 4;
    if (words <= 2 * 8) return 8;
    if (words <= 8 * 16) return 16;
    return 64;
}

// K14 and K15: what a shared-minibatch launch passes to its kernel.
constexpr int kXcds = 8;  // the hardware deals consecutive blocks to the XCDs in turn

struct SharedForwardArgs {
    const float* params;  // [n][L]
    const float* x;       // [B][width[0]]
    float* out;           // [n][B][width[layers]]
    int B;
    int tiles;   // batch tiles per member
    int blocks;  // n * tiles logical blocks
    long L;
    int layers;
    int has_bias;
    int width[kMaxLayers + 1];
    int act[kMaxLayers];
};

// The 16-byte word W[row][k0 .. k0+3] with everything past K zero; reads
// nothing outside the row.
__device__ __forceinline__ floatx4 shared_weight_word(const float* __restrict__ Wr, int K, int k0) {
    if (k0 + 4 <= K) return *reinterpret_cast<const floatx4_a4*>(Wr + k0);
    floatx4 w = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k0 < K) w.x = Wr[k0];
    if (k0 + 1 < K) w.y = Wr[k0 + 1];
    if (k0 + 2 < K) w.z = Wr[k0 + 2];
    return w;
}

// Checks a stack description (1 to kMaxLayers Linear layers, widths in
// [1, kMaxWidth], activation codes in range), copies it into width[0..layers]
// and act[0..layers) and returns the length of a member's flat vector:
// W_0 [D1][D0], b_0 [D1] (with biases), W_1, ... in named_parameters() order.
inline int64_t check_dense_stack(const std::vector<int64_t>& widths, const std::vector<int64_t>& activations,
                                 bool has_bias, int* width, int* act) {
    const int64_t layers = (int64_t)widths.size() - 1;
    TORCH_CHECK(layers >= 1 && layers <= kMaxLayers, "widths must describe 1 to ", kMaxLayers,
                " Linear layers (2 to ", kMaxLayers + 1, " entries), got ", widths.size(), " entries");
    TORCH_CHECK((int64_t)activations.size() == layers, "activations must have one code per layer (", layers,
                "), got ", activations.size());
    int64_t expected = 0;
    for (int64_t i = 0; i <= layers; ++i) {
        TORCH_CHECK(widths[i] >= 1 && widths[i] <= kMaxWidth, "widths[", i, "] must be in [1, ", kMaxWidth, "], got ",
                    widths[i]);
        width[i] = (int)widths[i];
    }
    for (int64_t i = 0; i < layers; ++i) {
        TORCH_CHECK(activations[i] >= kActIdentity && activations[i] <= kActRelu, "activations[", i,
                    "] must be 0 (identity), 1 (tanh) or 2 (ReLU), got ", activations[i]);
        act[i] = (int)activations[i];
        expected += widths[i + 1] * widths[i] + (has_bias ? widths[i + 1] : 0);
    }
    return expected;
}

// K16: what a weighted layer of a recurrent stack is.
enum PolicyLayerKind : int { kKindDense = 0, kKindRnn = 1, kKindLstm = 2 };

// check_dense_stack for a stack with exactly ONE recurrent layer: `kinds` has
// one code per layer; an RNN layer's activation is tanh or ReLU, an LSTM
// layer's is identity (its gates are fixed). Also copies the kinds into
// kind[0..layers), sets *recurrent to that layer's index and returns a
// member's length with the recurrent layer laid out as W_ih [R][K],
// W_hh [R][H], b_ih [R], b_hh [R], R = H (RNN) or 4H (LSTM, gates i, f, g, o).
inline int64_t check_recurrent_stack(const std::vector<int64_t>& kinds, const std::vector<int64_t>& widths,
                                     const std::vector<int64_t>& activations, bool has_bias, int* width, int* act,
                                     int* kind, int* recurrent) {
    check_dense_stack(widths, activations, has_bias, width, act);
    const int64_t layers = (int64_t)widths.size() - 1;
    TORCH_CHECK((int64_t)kinds.size() == layers, "kinds must have one code per layer (", layers, "), got ",
                kinds.size());
    int64_t expected = 0, found = 0;
    for (int64_t i = 0; i < layers; ++i) {
        TORCH_CHECK(kinds[i] >= kKindDense && kinds[i] <= kKindLstm, "kinds[", i,
                    "] must be 0 (dense), 1 (RNN) or 2 (LSTM), got ", kinds[i]);
        kind[i] = (int)kinds[i];
        const int64_t K = widths[i], N = widths[i + 1];
        if (kinds[i] == kKindDense) {
            expected += N * K + (has_bias ? N : 0);
            continue;
        }
        ++found;
        *recurrent = (int)i;
        if (kinds[i] == kKindRnn) {
            TORCH_CHECK(activations[i] == kActTanh || activations[i] == kActRelu, "activations[", i,
                        "] of an RNN layer must be 1 (tanh) or 2 (ReLU), got ", activations[i]);
        } else {
            TORCH_CHECK(activations[i] == kActIdentity, "activations[", i, "] of an LSTM layer must be 0, got ",
                        activations[i]);
        }
        const int64_t R = kinds[i] == kKindLstm ? 4 * N : N;
        expected += R * K + R * N + 2 * R;
    }
    TORCH_CHECK(found == 1, "kinds must hold exactly one recurrent layer, got ", found);
    return expected;
}

}  // namespace ea
