// What the population-batched dense-stack forwards share: K13
// (policy_forward.hip, every member on its own observation), K14
// (policy_forward_shared.hip, every member on one shared minibatch, fp32
// MFMA) and K15 (policy_forward_shared_bf16.hip, the same on bf16 MFMA).
#pragma once
#include <hip/hip_runtime.h>
#include <c10/util/Exception.h>

#include <cstdint>
#include <vector>

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

}  // namespace ea
