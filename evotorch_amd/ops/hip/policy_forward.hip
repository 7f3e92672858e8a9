// K13: population-batched forward of a dense policy stack (1 to 4 nn.Linear
// layers, each followed by identity, tanh or ReLU), fp32 throughout:
//
//   out[m] = act_{L-1}(W_{L-1} · ... act_0(W_0 · obs[m] + b_0) ... + b_{L-1})
//
// with member m's weights taken from its own flat vector params[m], laid out
// in named_parameters() order: W_0 [D1][D0] row-major, b_0 [D1] (if the stack
// has biases), W_1, ... This is models.Policy's per-step call for every
// environment that is not the fused synthetic rollout.
//
// The work is a GEMV chain per member: every weight is read exactly once and
// no operand is shared between members, so there is nothing for a matrix
// instruction to reuse. The kernel is bound by weight bandwidth and by the
// latency of the layer chain. (The shared-minibatch forward, where members
// do share an operand, is K14, policy_forward_shared.hip.)
//
// Work split
//   * A member is owned by ONE wave; a 256-thread block carries
//     kMembersPerBlock = 4 members. The member's activations live in two
//     ping-pong fp32 LDS buffers of that wave. Only the owning wave touches
//     them, so layers are separated by a wave-level fence and the kernel has
//     no block barrier at all (waves past the population's end just leave).
//   * Inside a layer (K inputs, N outputs) the wave is cut into 64/G row
//     groups of G lanes (G = 8, 16 or 64, picked per layer on the host from
//     K). A group computes one output row per pass: lane g of the group takes
//     the 16-byte words g, g + G, g + 2G, ... of the row, so the group reads
//     16·G contiguous bytes per step; the matching inputs come from LDS as
//     16-byte reads (every group reads the same addresses: a broadcast). The
//     K % 4 trailing elements go one each to the group's first lanes.
//   * The group's partial sums are added by DPP row shifts; its last lane
//     adds the bias, applies the activation and stores (LDS, or `out` for the
//     last layer).
//
// A member's rows are only 4-byte aligned (L and K are arbitrary); a global
// 16-byte load tolerates that (rollout_v7.hip relies on the same). A word is
// loaded only when it lies wholly inside its row, so nothing is read past a
// member's vector. Rows past N in the last pass recompute row N - 1 and drop
// the result: every lane stays active for the DPP sums and every address
// stays inside the member.
//
// Determinism: a member's output bits are a function of its params row, its
// obs row and the stack description alone. The summation order depends only
// on (K, G): lane order over words, x·y·z·w inside a word, the tail element,
// then the fixed DPP tree. Nothing depends on n, on the wave's place in the
// block or on other members. No atomics; all stores are plain vector stores.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "check.h"
#include "policy_common.h"
#include "reduce.h"
#include "rollout_common.h"

namespace ea {

constexpr int kMembersPerBlock = 4;  // one wave each

// The stack description travels by value in the kernel arguments.
struct PolicyForwardArgs {
    const float* params;  // [n][L]
    const float* obs;     // [n][width[0]]
    float* out;           // [n][width[layers]]
    int n;
    long L;
    int layers;
    int has_bias;
    int width[kMaxLayers + 1];
    int act[kMaxLayers];
    int group[kMaxLayers];  // lanes per row group: 8, 16 or 64
};

__global__ __launch_bounds__(kMembersPerBlock* kWaveSize) void population_mlp_forward_kernel(PolicyForwardArgs args) {
    // [wave][ping-pong][kMaxWidth]; 16-byte aligned for the ds_read_b128 of the inputs
    __shared__ __attribute__((aligned(16))) float lds[kMembersPerBlock][2][kMaxWidth];
    const int lane = threadIdx.x & (kWaveSize - 1);
    const int wave = threadIdx.x / kWaveSize;
    const int m = blockIdx.x * kMembersPerBlock + wave;
    if (m >= args.n) return;  // wave-uniform; the kernel has no block barrier

    float* cur = lds[wave][0];
    float* nxt = lds[wave][1];
    const int D0 = args.width[0];
    const float* obs = args.obs + (long)m * D0;
    for (int k = lane; k < D0; k += kWaveSize) cur[k] = obs[k];
    wave_lds_fence();

    const float* p = args.params + (long)m * args.L;
    for (int l = 0; l < args.layers; ++l) {
        const int K = args.width[l], N = args.width[l + 1];
        const float* W = p;
        p += (long)N * K;
        const float* b = nullptr;
        if (args.has_bias) {
            b = p;
            p += N;
        }
        const bool last = l + 1 == args.layers;
        float* y = last ? args.out + (long)m * N : nxt;
        const int G = args.group[l];
        if (G == 8) {
            policy_layer<8>(W, b, cur, y, K, N, args.act[l], lane);
        } else if (G == 16) {
            policy_layer<16>(W, b, cur, y, K, N, args.act[l], lane);
        } else {
            policy_layer<64>(W, b, cur, y, K, N, args.act[l], lane);
        }
        if (!last) {
            wave_lds_fence();
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
    }
}

torch::Tensor population_mlp_forward(torch::Tensor params, torch::Tensor obs, std::vector<int64_t> widths,
                                     std::vector<int64_t> activations, bool has_bias) {
    check_primary(params, "params", 2);
    TORCH_CHECK(params.scalar_type() == torch::kFloat32, "params must be float32, got ", params.scalar_type());
    PolicyForwardArgs args{};
    const int64_t expected = check_dense_stack(widths, activations, has_bias, args.width, args.act);
    const int64_t layers = (int64_t)widths.size() - 1;
    for (int64_t i = 0; i < layers; ++i) args.group[i] = policy_group_width(args.width[i]);
    const int64_t n = params.size(0), L = params.size(1);
    TORCH_CHECK(L == expected, "params must hold ", expected, " values per member for this stack, got L = ", L);
    TORCH_CHECK(n <= INT_MAX / kMaxWidth, "params: too many members (", n, ")");
    check_operand(obs, "obs", params, n * widths[0]);

    torch::Tensor out = torch::empty({n, widths[layers]}, params.options());
    if (n == 0) return out;
    args.params = params.data_ptr<float>();
    args.obs = obs.data_ptr<float>();
    args.out = out.data_ptr<float>();
    args.n = (int)n;
    args.L = (long)L;
    args.layers = (int)layers;
    args.has_bias = has_bias ? 1 : 0;
    const int blocks = (int)((n + kMembersPerBlock - 1) / kMembersPerBlock);
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(population_mlp_forward_kernel, dim3(blocks), dim3(kMembersPerBlock * kWaveSize), 0, stream,
                       args);
    return out;
}

}  // namespace ea
