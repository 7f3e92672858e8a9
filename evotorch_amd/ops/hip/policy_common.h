// What the two population-batched dense-stack forwards share: K13
// (policy_forward.hip, every member on its own observation) and K14
// (policy_forward_shared.hip, every member on one shared minibatch).
#pragma once
#include <hip/hip_runtime.h>
#include <c10/util/Exception.h>

#include <cstdint>
#include <vector>

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
