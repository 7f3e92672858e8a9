// K14: population-batched forward of a dense stack (1 to 4 nn.Linear layers,
// each followed by identity, tanh or ReLU) on ONE shared minibatch, fp32
// throughout, on the fp32 matrix instruction v_mfma_f32_16x16x4_f32:
//
//   out[m] = act_{L-1}(... act_0(X · W_0[m]^T + b_0[m]) ... · W_{L-1}[m]^T + b_{L-1}[m])
//
// with X [B][D0] the same for every member m and member m's weights taken
// from its flat vector params[m] (K13's layout: W_0 [D1][D0] row-major, b_0,
// W_1, ... in named_parameters() order). This is SupervisedNE's
// common-minibatch evaluation. Unlike K13 the work is a real GEMM chain per
// member, so a weight fetched into a register is reused by every batch row
// of the tile, and the hidden activations never leave LDS.
//
// Work split
//   * One 256-thread block per (member, batch tile of BT rows); BT = 16, 32
//     or 64 is a template parameter, picked on the host from the widths alone
//     (shared_batch_tile). Consecutive logical blocks are the tiles of one
//     member, and the grid is dealt to logical blocks so that the blocks the
//     hardware sends to one XCD (every 8th) are consecutive logical blocks:
//     a member's weights are re-read from that XCD's L2. (The map is a
//     bijection, so only the locality, not the result, rests on that dealing;
//     it was not measured against the plain order.)
//   * Activations live in two LDS buffers, rows of one batch element each.
//     Buffer 0 holds the widths D0, D2, ... and buffer 1 holds D1, D3, ...;
//     each has its own row stride, the widest of its widths rounded up to 16
//     plus 4 floats (shared_stride). The last layer stores to `out`.
//   * A layer (K inputs, N outputs) is cut into 16-column output tiles, dealt
//     round-robin to the 4 waves. For a column tile a wave holds BT/16
//     accumulators (one per 16-row tile) and walks K in super-steps of 16:
//     lane l (g = l / 16, j = l % 16) loads the 16-byte weight word
//     W[col0 + j][16s + 4g .. +3] from global memory and, per row tile, the
//     16-byte LDS word act[row0 + j][16s + 4g .. +3]; component i of both
//     feeds the i-th of four MFMAs, so MFMA i sums k = 16s + 4g + i over
//     g = 0..3. The k index is permuted the same way in A and B, which a sum
//     allows. Weight words are fetched kPrefetch super-steps ahead.
//   * Epilogue: the D fragment is rows 4g .. 4g+3, column j. Bias, then
//     activation, then a store to the other LDS buffer (columns past N store
//     0, so the next layer's K padding is zero) or, for the last layer, to
//     out[m][b][col] for b < B and col < N. One block barrier per layer.
//
// Alignment and bounds: a member's rows are only 4-byte aligned; a global
// 16-byte load tolerates that (as in K13 and v7). A weight word is loaded
// only when it lies wholly inside its row, the K % 4 tail elements singly,
// everything past K is zero and touches no memory. Output columns past N
// recompute column N - 1 and drop the result, so no address leaves the
// member's vector. Rows past B hold zero inputs and are never stored.
//
// LDS banks: with a row stride of 16a + 4 floats the 16 rows of a fragment
// read (16 bytes each, at the same column) fall on 16 different 16-byte bank
// groups, and the epilogue's stores of rows 4g + r, column j fall on banks
// 16g + j.
//
// Determinism: out[m, b, :] is a function of params[m], x[b] and the stack
// description alone. Row i of an MFMA result depends on row i of A only, the
// k order is a fixed function of K, and BT depends on the widths only, so
// neither n, B, the row's place in its tile nor the other members matter.
// No atomics; all stores are plain vector stores.
//
// K17 (kLoss): the last layer stores its tile to the other LDS buffer instead
// of `out`, and after one barrier the loss phase of policy_loss.h reduces it
// to the member's loss. Up to that store the arithmetic is the same code, so
// the loss is taken of the bits the kLoss = false kernel stores.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "check.h"
#include "policy_common.h"
#include "policy_loss.h"
#include "rollout_common.h"

namespace ea {

constexpr int kSharedThreads = 256;
constexpr int kSharedWaves = kSharedThreads / 64;
constexpr int kPrefetch = 4;  // weight words in flight per lane, in super-steps
// two blocks share a CU's 160 KB of LDS while each stays within this
constexpr size_t kSharedLdsPerBlock = 80 * 1024;

// The LDS layout, stated once for the kernel's carve-up and the launcher's
// footprint: buffer 0 [bt][shared_stride(.., 0)] floats, then buffer 1
// [bt][shared_stride(.., 1)]. Buffer `parity` holds the inputs of the layers
// parity, parity + 2, ...; its row stride is the widest of them rounded up to
// 16, plus 4 floats. (Plain ints on purpose: a layout struct whose strides
// the layer loop picks by l & 1 ends up in scratch.)
__host__ __device__ inline int shared_stride(const int* width, int layers, int parity) {
    int widest = 1;
    for (int i = parity; i < layers; i += 2) widest = width[i] > widest ? width[i] : widest;
    return ((widest + 15) & ~15) + 4;
}

__host__ __device__ inline size_t shared_lds_bytes(const int* width, int layers, int bt) {
    return (size_t)bt * (shared_stride(width, layers, 0) + shared_stride(width, layers, 1)) * sizeof(float);
}

// The loss layout (K17) is the same rule with the last layer's output counted
// as one more row to hold: buffer layers & 1 also fits width[layers].
__host__ __device__ inline int shared_loss_stride(const int* width, int layers, int parity) {
    return shared_stride(width, layers + 1, parity);
}

__host__ __device__ inline size_t shared_loss_lds_bytes(const int* width, int layers, int bt) {
    return shared_lds_bytes(width, layers + 1, bt);
}

template <int BT, bool kLoss>
__global__ __launch_bounds__(kSharedThreads) void population_mlp_forward_shared_kernel(SharedForwardArgs args,
                                                                                       SharedLossArgs largs) {
    constexpr int kRowTiles = BT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char shared_lds[];
    // grid block -> logical block: XCD x takes the logical blocks [x * per_xcd, (x + 1) * per_xcd)
    const int per_xcd = (args.blocks + kXcds - 1) / kXcds;
    const int logical = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
    if (logical >= args.blocks) return;  // block-uniform, before any barrier
    const int m = logical / args.tiles;
    const int b0 = (logical - m * args.tiles) * BT;

    const int stride0 = kLoss ? shared_loss_stride(args.width, args.layers, 0) : shared_stride(args.width, args.layers, 0);
    const int stride1 = kLoss ? shared_loss_stride(args.width, args.layers, 1) : shared_stride(args.width, args.layers, 1);
    float* const buf0 = reinterpret_cast<float*>(shared_lds);
    float* const buf1 = buf0 + BT * stride0;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;

    // x tile into buffer 0: rows past B and columns up to the next multiple of 16 are zero
    {
        const int D0 = args.width[0], D0p = (D0 + 15) & ~15;
        for (int r = wave; r < BT; r += kSharedWaves) {
            const int b = b0 + r;
            const float* xr = args.x + (long)min(b, args.B - 1) * D0;
            for (int c = lane; c < D0p; c += 64) buf0[r * stride0 + c] = (b < args.B && c < D0) ? xr[c] : 0.0f;
        }
    }
    __syncthreads();

    const float* p = args.params + (long)m * args.L;
    for (int l = 0; l < args.layers; ++l) {
        const int K = args.width[l], N = args.width[l + 1], act = args.act[l];
        const float* W = p;
        p += (long)N * K;
        const float* bias = nullptr;
        if (args.has_bias) {
            bias = p;
            p += N;
        }
        const bool last = l + 1 == args.layers;
        const bool odd = l & 1;
        const float* cur = odd ? buf1 : buf0;
        float* nxt = odd ? buf0 : buf1;
        const int cs = odd ? stride1 : stride0, ns = odd ? stride0 : stride1;
        const int steps = (K + 15) >> 4;
        const int col_tiles = (N + 15) >> 4;
        for (int ct = wave; ct < col_tiles; ct += kSharedWaves) {
            const int col = ct * 16 + j;
            const int colc = min(col, N - 1);
            const float* Wr = W + (long)colc * K;
            floatx4 acc[kRowTiles];
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) acc[t] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
            floatx4 w[kPrefetch];
#pragma unroll
            for (int u = 0; u < kPrefetch; ++u) w[u] = shared_weight_word(Wr, K, 16 * u + 4 * g);
            for (int s0 = 0; s0 < steps; s0 += kPrefetch) {
#pragma unroll
                for (int u = 0; u < kPrefetch; ++u) {
                    const int s = s0 + u;
                    const floatx4 wv = w[u];
                    w[u] = shared_weight_word(Wr, K, 16 * (s + kPrefetch) + 4 * g);
                    if (s < steps) {  // wave-uniform
                        floatx4 a[kRowTiles];
#pragma unroll
                        for (int t = 0; t < kRowTiles; ++t)
                            a[t] = *reinterpret_cast<const floatx4*>(cur + (t * 16 + j) * cs + 16 * s + 4 * g);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
#pragma unroll
                            for (int t = 0; t < kRowTiles; ++t)
                                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i], wv[i], acc[t], 0, 0, 0);
                        }
                    }
                }
            }
            const float bv = bias != nullptr ? bias[colc] : 0.0f;
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = t * 16 + 4 * g + r;
                    float v = acc[t][r];
                    if (bias != nullptr) v += bv;
                    v = policy_activation(v, act);
                    if (last) {
                        if constexpr (kLoss) {
                            if (col < N) nxt[row * ns + col] = v;
                        } else {
                            const int b = b0 + row;
                            if (b < args.B && col < N) args.out[((long)m * args.B + b) * N + col] = v;
                        }
                    } else {
                        nxt[row * ns + col] = col < N ? v : 0.0f;
                    }
                }
            }
        }
        if (!last) __syncthreads();
    }
    if constexpr (kLoss) {
        __syncthreads();
        const bool odd = args.layers & 1;  // the buffer the last layer stored to
        shared_loss_phase<BT>(odd ? buf1 : buf0, odd ? stride1 : stride0, odd ? buf0 : buf1, m, b0 / BT, args, largs);
    }
}

// Rows per batch tile, from the widths alone: the largest tile whose two
// buffers leave room for a second block on the CU; stacks too wide for that
// at any size take 16 rows (131,584 bytes at most, one block per CU).
static int shared_batch_tile(const int* width, int layers) {
    for (int bt : {64, 32})
        if (shared_lds_bytes(width, layers, bt) <= kSharedLdsPerBlock) return bt;
    return 16;
}

// The same rule asked of the loss layout.
int shared_loss_batch_tile(const int* width, int layers) { return shared_batch_tile(width, layers + 1); }

// What the router asks (models/functional.py sends only stacks with tiles of
// 32 rows or more here: with 16-row tiles the kernel measured slower than
// the batched-GEMM path, see docs/kernels.md).
int64_t population_mlp_forward_shared_batch_tile(std::vector<int64_t> widths) {
    int width[kMaxLayers + 1], act[kMaxLayers];
    const std::vector<int64_t> identity(widths.empty() ? 0 : widths.size() - 1, kActIdentity);
    check_dense_stack(widths, identity, false, width, act);
    return shared_batch_tile(width, (int)widths.size() - 1);
}

template <int BT, bool kLoss>
static void launch_shared(const SharedForwardArgs& args, const SharedLossArgs& largs, size_t lds_bytes,
                          hipStream_t stream) {
    static bool attr_set = false;
    if (!attr_set) {
        allow_max_dynamic_lds(reinterpret_cast<const void*>(&population_mlp_forward_shared_kernel<BT, kLoss>));
        attr_set = true;
    }
    const int grid = (args.blocks + kXcds - 1) / kXcds * kXcds;
    hipLaunchKernelGGL((population_mlp_forward_shared_kernel<BT, kLoss>), dim3(grid), dim3(kSharedThreads), lds_bytes,
                       stream, args, largs);
}

// K17's launch: `args` as for the forward (out unused), `bt` from shared_loss_batch_tile.
void launch_shared_loss(const SharedForwardArgs& args, const SharedLossArgs& largs, int bt, hipStream_t stream) {
    const size_t lds_bytes = shared_loss_lds_bytes(args.width, args.layers, bt);
    if (bt == 64) {
        launch_shared<64, true>(args, largs, lds_bytes, stream);
    } else if (bt == 32) {
        launch_shared<32, true>(args, largs, lds_bytes, stream);
    } else {
        launch_shared<16, true>(args, largs, lds_bytes, stream);
    }
}

torch::Tensor population_mlp_forward_shared(torch::Tensor params, torch::Tensor x, std::vector<int64_t> widths,
                                            std::vector<int64_t> activations, bool has_bias) {
    check_primary(params, "params", 2);
    TORCH_CHECK(params.scalar_type() == torch::kFloat32, "params must be float32, got ", params.scalar_type());
    SharedForwardArgs args{};
    const int64_t expected = check_dense_stack(widths, activations, has_bias, args.width, args.act);
    const int64_t layers = (int64_t)widths.size() - 1;
    const int64_t n = params.size(0), L = params.size(1);
    TORCH_CHECK(L == expected, "params must hold ", expected, " values per member for this stack, got L = ", L);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == widths[0], "x must be 2-D (B, ", widths[0], "), got ", x.sizes());
    const int64_t B = x.size(0);
    check_operand(x, "x", params, B * widths[0]);
    const int bt = shared_batch_tile(args.width, (int)layers);
    const int64_t tiles = (B + bt - 1) / bt;
    TORCH_CHECK(B <= INT_MAX - 64, "x: too many rows (", B, ")");
    TORCH_CHECK(n * tiles <= INT_MAX - kXcds, "params, x: too many (member, batch tile) blocks (", n * tiles, ")");

    torch::Tensor out = torch::empty({n, B, widths[layers]}, params.options());
    if (n == 0 || B == 0) return out;
    args.params = params.data_ptr<float>();
    args.x = x.data_ptr<float>();
    args.out = out.data_ptr<float>();
    args.B = (int)B;
    args.tiles = (int)tiles;
    args.blocks = (int)(n * tiles);
    args.L = (long)L;
    args.layers = (int)layers;
    args.has_bias = has_bias ? 1 : 0;
    const size_t lds_bytes = shared_lds_bytes(args.width, args.layers, bt);
    auto stream = at::cuda::getCurrentCUDAStream();
    const SharedLossArgs no_loss{};
    if (bt == 64) {
        launch_shared<64, false>(args, no_loss, lds_bytes, stream);
    } else if (bt == 32) {
        launch_shared<32, false>(args, no_loss, lds_bytes, stream);
    } else {
        launch_shared<16, false>(args, no_loss, lds_bytes, stream);
    }
    return out;
}

}  // namespace ea
