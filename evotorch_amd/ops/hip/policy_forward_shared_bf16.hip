// K15: K14's shared-minibatch population forward with bf16 operands on
// v_mfma_f32_16x16x32_bf16, for stacks too wide for K14's fp32 LDS rows:
//
//   h_0 = X,  h_{l+1} = act_l(bf16(h_l) · bf16(W_l[m])^T + b_l[m]),  out[m] = h_layers
//
// X [B][D0] is the same for every member m; member m's weights come from its
// flat fp32 vector params[m] (K13's layout). Each weight, each x element and
// each hidden activation is rounded to bf16 once (nearest even, NaN stays
// NaN); products are summed in fp32, bias and activation are fp32, and the
// last layer's result is stored unrounded. Opt-in: the caller asks for bf16.
//
// What bf16 buys over K14 at 784 -> 128 -> 10 (K14: 16-row tiles, 0.42x the
// batched-GEMM path):
//   * an LDS row is half as long, so the batch tile is 32 rows (64 fit), not
//     16, and two blocks still share a CU;
//   * a lane's weight fragment (8 consecutive k of one output column) feeds
//     BT/16 MFMAs of K = 32 each: 8 fp32 loaded per 2 MFMAs, where K14 loads
//     4 fp32 per 4 MFMAs of K = 4 (a 16th of the matrix instructions per
//     weight);
//   * a member's weights are re-read for 4 tiles at B = 128, not 8.
//
// Work split
//   * One 256-thread block per (member, batch tile of BT rows), BT a template
//     parameter picked on the host from the widths alone (bf16_batch_tile: 32
//     rows for every stack; the 64-row instantiation is kept for measuring). K14's grid order: consecutive logical blocks are the
//     tiles of one member, dealt so that one XCD (every 8th grid block) gets
//     consecutive logical blocks and re-reads a member's weights from its L2.
//   * Two bf16 LDS buffers of BT rows: buffer 0 holds the inputs of the even
//     layers, buffer 1 those of the odd layers, each with its own row stride:
//     the widest of its widths rounded up to 32, plus 8 elements
//     (64a + 16 bytes). The x tile is converted once while it is staged.
//   * A layer (K inputs, N outputs) is cut into 16-column output tiles, dealt
//     round-robin to the 4 waves. For a column tile a wave holds BT/16
//     accumulators and walks K in steps of 32: lane l (g = l / 16, j = l % 16)
//     loads the 8 fp32 W[col0 + j][32s + 8g .. +7] from global memory as two
//     16-byte words, converts them to one B fragment (4 v_cvt_pk_bf16_f32)
//     and, per row tile, reads the A fragment act[row0 + j][32s + 8g .. +7]
//     (16 bytes) from LDS: the lane mapping of rollout_v7.hip. Weight words
//     are fetched kBf16Prefetch steps ahead.
//   * Epilogue: the D fragment is rows 4g .. 4g+3, column j. The fp32 bias is
//     the accumulator's initial value, so the sum is b + Σ products in fp32
//     and the epilogue has no add. Activation, then for a hidden layer a pairwise conversion (rows 4g + {0,1}, {2,3})
//     and 2-byte stores to the other buffer, or for the last layer fp32 stores
//     to out[m][b][col] for b < B and col < N. One block barrier per layer.
//
// Padding and bounds: a layer reads K rounded up to 32 columns of its input
// buffer, so the staging zeroes x's columns up to that, and a hidden layer
// writes column tiles up to N rounded up to 32; a tile that lies wholly past
// N (and every column past N) stores 0 and loads no weights. A weight word
// is loaded only when it lies wholly inside its row (rows are 4-byte aligned,
// which a global 16-byte load tolerates), the K % 4 tail singly, everything
// past K is zero and touches no memory. Columns past N in a partial tile
// recompute column N - 1 and drop the result. Rows past B hold zero inputs
// and are never stored.
//
// LDS banks: with a row stride of 64a + 16 bytes the 16 rows of a fragment
// read (16 bytes each, same column) fall on 16 different 16-byte bank groups.
//
// Determinism: out[m, b, :] is a function of params[m], x[b] and the stack
// description alone: row i of an MFMA result depends on row i of A only, the
// k order is a fixed function of K, BT depends on the widths only. No
// atomics; all stores are plain vector stores; current stream, no host sync.
//
// K17 (kLoss): the last layer stores its unrounded fp32 tile to the other LDS
// buffer, whose rows are long enough for it (bf16_loss_stride), instead of
// `out`, and after one barrier the loss phase of policy_loss.h reduces it to
// the member's loss: the loss of the bits the kLoss = false kernel stores.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "check.h"
#include "policy_common.h"
#include "policy_loss.h"
#include "rollout_common.h"

namespace ea {

constexpr int kBf16Threads = 256;
constexpr int kBf16Waves = kBf16Threads / 64;
constexpr int kBf16Prefetch = 4;  // weight steps (32 bytes per lane each) in flight
constexpr size_t kBf16LdsOneBlock = 160 * 1024;  // a CU's LDS; two blocks share it while each stays within half

typedef __attribute__((ext_vector_type(2))) float floatx2;
typedef __attribute__((ext_vector_type(8))) float floatx8;

// The LDS layout, stated once for the kernel and the launcher: buffer 0
// [bt][bf16_stride(.., 0)] bf16, then buffer 1 [bt][bf16_stride(.., 1)].
// Buffer `parity` holds the inputs of the layers parity, parity + 2, ...
__host__ __device__ inline int bf16_stride(const int* width, int layers, int parity) {
    int widest = 1;
    for (int i = parity; i < layers; i += 2) widest = width[i] > widest ? width[i] : widest;
    return ((widest + 31) & ~31) + 8;
}

__host__ __device__ inline size_t bf16_lds_bytes(const int* width, int layers, int bt) {
    return (size_t)bt * (bf16_stride(width, layers, 0) + bf16_stride(width, layers, 1)) * sizeof(__bf16);
}

// The loss layout (K17): buffer layers & 1 also holds the last layer's output
// as one fp32 row of width[layers], i.e. 2 * width[layers] bf16 slots, padded
// by the same rule (rows stay 64a + 16 bytes, so 16-byte aligned).
__host__ __device__ inline int bf16_loss_stride(const int* width, int layers, int parity) {
    const int s = bf16_stride(width, layers, parity);
    const int row = ((2 * width[layers] + 31) & ~31) + 8;
    return parity == (layers & 1) && row > s ? row : s;
}

__host__ __device__ inline size_t bf16_loss_lds_bytes(const int* width, int layers, int bt) {
    return (size_t)bt * (bf16_loss_stride(width, layers, 0) + bf16_loss_stride(width, layers, 1)) * sizeof(__bf16);
}

template <int BT, bool kLoss>
__global__ __launch_bounds__(kBf16Threads) void population_mlp_forward_shared_bf16_kernel(SharedForwardArgs args,
                                                                                          SharedLossArgs largs) {
    constexpr int kRowTiles = BT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char bf16_lds[];
    // grid block -> logical block: XCD x takes the logical blocks [x * per_xcd, (x + 1) * per_xcd)
    const int per_xcd = (args.blocks + kXcds - 1) / kXcds;
    const int logical = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
    if (logical >= args.blocks) return;  // block-uniform, before any barrier
    const int m = logical / args.tiles;
    const int b0 = (logical - m * args.tiles) * BT;

    const int stride0 = kLoss ? bf16_loss_stride(args.width, args.layers, 0) : bf16_stride(args.width, args.layers, 0);
    const int stride1 = kLoss ? bf16_loss_stride(args.width, args.layers, 1) : bf16_stride(args.width, args.layers, 1);
    __bf16* const buf0 = reinterpret_cast<__bf16*>(bf16_lds);
    __bf16* const buf1 = buf0 + BT * stride0;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;

    // x tile into buffer 0, converted in pairs: rows past B and columns up to the next multiple of 32 are zero
    {
        const int D0 = args.width[0], pairs = ((D0 + 31) & ~31) >> 1;
        for (int r = wave; r < BT; r += kBf16Waves) {
            const int b = b0 + r;
            const float* xr = args.x + (long)min(b, args.B - 1) * D0;
            bf16x2* row = reinterpret_cast<bf16x2*>(buf0 + r * stride0);
            for (int c2 = lane; c2 < pairs; c2 += 64) {
                const int c = 2 * c2;
                floatx2 v = {0.0f, 0.0f};
                if (b < args.B && c < D0) v.x = xr[c];
                if (b < args.B && c + 1 < D0) v.y = xr[c + 1];
                row[c2] = __builtin_convertvector(v, bf16x2);
            }
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
        const __bf16* cur = odd ? buf1 : buf0;
        __bf16* nxt = odd ? buf0 : buf1;
        const int cs = odd ? stride1 : stride0, ns = odd ? stride0 : stride1;
        // a hidden layer also writes the zero tiles that pad its output to a multiple of 32
        const int col_tiles = last ? (N + 15) >> 4 : ((N + 31) >> 5) * 2;
        for (int ct = wave; ct < col_tiles; ct += kBf16Waves) {
            const int col = ct * 16 + j;
            const int colc = min(col, N - 1);
            const float* Wr = W + (long)colc * K;
            const int Kt = ct * 16 < N ? K : 0;  // wave-uniform: a padding tile loads and multiplies nothing
            const int full = Kt >> 5;  // steps whose 32 columns lie wholly inside the row
            // the fp32 bias is the accumulators' first term: no add left for the epilogue
            const float bv = bias != nullptr ? bias[colc] : 0.0f;
            floatx4 acc[kRowTiles];
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) acc[t] = floatx4{bv, bv, bv, bv};
            // one step: the lane's 8 weights to a B fragment, BT/16 A fragments from LDS, BT/16 MFMAs
            auto step = [&](floatx4 lo, floatx4 hi, int s) __attribute__((always_inline)) {
                const floatx8 w8 = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                const bf16x8 bw = __builtin_convertvector(w8, bf16x8);
                bf16x8 a[kRowTiles];
#pragma unroll
                for (int t = 0; t < kRowTiles; ++t)
                    a[t] = *reinterpret_cast<const bf16x8*>(cur + (t * 16 + j) * cs + 32 * s + 8 * g);
#pragma unroll
                for (int t = 0; t < kRowTiles; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], bw, acc[t], 0, 0, 0);
            };
            // The full steps are loaded without a branch, kBf16Prefetch ahead; the look-ahead past
            // the last full step re-reads that step, so no address leaves the row and the loop body
            // holds no divergent load (one would make every wait a wait for all loads in flight).
            // The K % 32 tail step is loaded element-wise where a word crosses the row's end (zero
            // past K, nothing read), behind the first prefetches, and used last.
            const floatx4_a4* Wg = reinterpret_cast<const floatx4_a4*>(Wr + 8 * g);
            floatx4 wlo[kBf16Prefetch], whi[kBf16Prefetch];
            if (full > 0) {
#pragma unroll
                for (int u = 0; u < kBf16Prefetch; ++u) {
                    const int su = min(u, full - 1);
                    wlo[u] = Wg[8 * su];
                    whi[u] = Wg[8 * su + 1];
                }
            }
            const floatx4 tlo = shared_weight_word(Wr, Kt, 32 * full + 8 * g);
            const floatx4 thi = shared_weight_word(Wr, Kt, 32 * full + 8 * g + 4);
            if (full > 0) {
                for (int s0 = 0; s0 < full; s0 += kBf16Prefetch) {
#pragma unroll
                    for (int u = 0; u < kBf16Prefetch; ++u) {
                        const int s = s0 + u;
                        const floatx4 lo = wlo[u], hi = whi[u];
                        const int sn = min(s + kBf16Prefetch, full - 1);
                        wlo[u] = Wg[8 * sn];
                        whi[u] = Wg[8 * sn + 1];
                        if (s < full) step(lo, hi, s);  // wave-uniform
                    }
                }
            }
            if (Kt & 31) step(tlo, thi, full);  // wave-uniform
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) {
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const int row = t * 16 + 4 * g + r;
                    floatx2 v = {policy_activation(acc[t][r], act), policy_activation(acc[t][r + 1], act)};
                    if (last && kLoss) {
                        if (col < N) {  // fp32 rows of ns / 2 floats in the other buffer
                            float* tile = reinterpret_cast<float*>(nxt);
                            tile[row * (ns >> 1) + col] = v.x;
                            tile[(row + 1) * (ns >> 1) + col] = v.y;
                        }
                    } else if (last) {
                        if (col < N) {
                            if (b0 + row < args.B) args.out[((long)m * args.B + b0 + row) * N + col] = v.x;
                            if (b0 + row + 1 < args.B) args.out[((long)m * args.B + b0 + row + 1) * N + col] = v.y;
                        }
                    } else {
                        if (col >= N) v = floatx2{0.0f, 0.0f};
                        const bf16x2 h = __builtin_convertvector(v, bf16x2);
                        nxt[row * ns + col] = h.x;
                        nxt[(row + 1) * ns + col] = h.y;
                    }
                }
            }
        }
        if (!last) __syncthreads();
    }
    if constexpr (kLoss) {
        __syncthreads();
        const bool odd = args.layers & 1;  // the buffer the last layer stored to
        shared_loss_phase<BT>(reinterpret_cast<const float*>(odd ? buf1 : buf0), (odd ? stride1 : stride0) >> 1,
                              reinterpret_cast<float*>(odd ? buf0 : buf1), m, b0 / BT, args, largs);
    }
}

// Rows per batch tile, from the widths alone. 32 for every stack: measured
// against 64 rows (docs/kernels.md) it ties or loses by 8 % at n = 1024,
// B = 128 on narrow stacks and wins by 1.3x to 1.8x everywhere else (B = 32,
// n = 64, and 784 -> 128 -> 10 at any size, where 64 rows leave one block per
// CU). 32 rows of two 1024-wide buffers are 132,096 bytes, so the tile always
// fits, and two blocks share a CU while a block stays within 80 KB.
static int bf16_batch_tile(const int* width, int layers) {
    (void)width, (void)layers;
    return 32;
}

// The loss layout's tile: 32 rows as above, except where a very wide last
// layer's fp32 row next to a wide input no longer fits a CU's LDS at 32 rows
// (more than 160 KB, e.g. 1024 -> 1024 -> 1024: 197,632 bytes); those take 16.
int bf16_loss_batch_tile(const int* width, int layers) {
    return bf16_loss_lds_bytes(width, layers, 32) <= kBf16LdsOneBlock ? 32 : 16;
}

int64_t population_mlp_forward_shared_bf16_batch_tile(std::vector<int64_t> widths) {
    int width[kMaxLayers + 1], act[kMaxLayers];
    const std::vector<int64_t> identity(widths.empty() ? 0 : widths.size() - 1, kActIdentity);
    check_dense_stack(widths, identity, false, width, act);
    return bf16_batch_tile(width, (int)widths.size() - 1);
}

template <int BT, bool kLoss>
static void launch_shared_bf16(const SharedForwardArgs& args, const SharedLossArgs& largs, size_t lds_bytes,
                               hipStream_t stream) {
    static bool attr_set = false;
    if (!attr_set) {
        allow_max_dynamic_lds(reinterpret_cast<const void*>(&population_mlp_forward_shared_bf16_kernel<BT, kLoss>));
        attr_set = true;
    }
    const int grid = (args.blocks + kXcds - 1) / kXcds * kXcds;
    hipLaunchKernelGGL((population_mlp_forward_shared_bf16_kernel<BT, kLoss>), dim3(grid), dim3(kBf16Threads),
                       lds_bytes, stream, args, largs);
}

// K17's launch: `args` as for the forward (out unused), `bt` from bf16_loss_batch_tile.
void launch_shared_loss_bf16(const SharedForwardArgs& args, const SharedLossArgs& largs, int bt, hipStream_t stream) {
    const size_t lds_bytes = bf16_loss_lds_bytes(args.width, args.layers, bt);
    if (bt == 32) {
        launch_shared_bf16<32, true>(args, largs, lds_bytes, stream);
    } else {
        launch_shared_bf16<16, true>(args, largs, lds_bytes, stream);
    }
}

// `batch_tile` 0 takes the rule above; 32 or 64 overrides it (for measuring
// the rule; the op never passes it, so its results keep one tile per stack).
torch::Tensor population_mlp_forward_shared_bf16(torch::Tensor params, torch::Tensor x, std::vector<int64_t> widths,
                                                 std::vector<int64_t> activations, bool has_bias,
                                                 int64_t batch_tile) {
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
    TORCH_CHECK(batch_tile == 0 || batch_tile == 32 || batch_tile == 64, "batch_tile must be 0, 32 or 64, got ",
                batch_tile);
    const int bt = batch_tile == 0 ? bf16_batch_tile(args.width, (int)layers) : (int)batch_tile;
    const size_t lds_bytes = bf16_lds_bytes(args.width, (int)layers, bt);
    TORCH_CHECK(lds_bytes <= kBf16LdsOneBlock, "batch_tile ", bt, " needs ", lds_bytes, " bytes of LDS for these widths");
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
    auto stream = at::cuda::getCurrentCUDAStream();
    const SharedLossArgs no_loss{};
    if (bt == 64) {
        launch_shared_bf16<64, false>(args, no_loss, lds_bytes, stream);
    } else {
        launch_shared_bf16<32, false>(args, no_loss, lds_bytes, stream);
    }
    return out;
}

}  // namespace ea
