// K17: the loss phase that K14 (policy_forward_shared.hip) and K15
// (policy_forward_shared_bf16.hip) run in their last epilogue when they are
// instantiated with kLoss: the last layer's tile stays in LDS as fp32 rows,
// is reduced here to the member's mean MSE or cross-entropy, and the block
// writes one float instead of BT * D_last.
//
// Work split (256 threads, the forward's block)
//   * Wave w takes the rows [w * BT/4, (w + 1) * BT/4) of the tile. A row is
//     given to a group of G lanes, G = 16 for D_last <= 64 (four rows per wave
//     pass, at most four columns per lane) and G = 64 for wider rows; the host
//     picks G from D_last (shared_loss_group), K13's group idea.
//   * MSE: a lane sums (v[c] - y[b][c])^2 over its columns c = gl, gl + G, ...
//     in order; the DPP tree of group_sum<G> leaves the row's sum in the
//     group's last lane. y is read from global memory once.
//   * Cross-entropy: the lanes' maxima meet in an xor butterfly (a maximum is
//     exact, so its order is free), then a lane sums expf(v[c] - max) over its
//     columns in order, group_sum<G> again, and the group's last lane forms
//     (logf(sum) + max) - v[target]. expf and logf are the accurate ones.
//   * The group's last lane adds its rows in order; the (up to) four groups of
//     a wave are added in lane order, the four waves in wave order by thread
//     0, which divides by the divisor and stores. Rows b >= B add nothing.
//
// ignore_index: a row whose target is -100 adds nothing, and the divisor is
// the number of targets != -100 in the WHOLE of y, which every block counts
// for itself (B int64 reads, ballot + popcount, exact). All ignored: 0/0 =
// NaN, as torch gives. Any other target outside [0, C) makes the row's loss
// NaN and indexes nothing.
//
// Determinism: the order above is a fixed function of the stack, B and BT,
// so loss[m] depends bit for bit on params[m], x, y and the stack only. No
// atomics, no tickets; plain vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include "policy_common.h"

namespace ea {

enum SharedLossKind : int { kLossMse = 0, kLossCrossEntropy = 1 };
constexpr long long kLossIgnoreIndex = -100;  // nn.CrossEntropyLoss's default

struct SharedLossArgs {
    const float* y_mse;     // [B][width[layers]], kLossMse
    const long long* y_ce;  // [B], kLossCrossEntropy
    float* loss;            // [n][tiles]: the tile's sum over the divisor
    int kind;
    int group;  // lanes per row: 16 or 64
};

// Lanes per tile row, from the row's length alone.
inline int shared_loss_group(int d_last) { return d_last <= 64 ? 16 : 64; }

// What the kernel files provide to the entry point (policy_loss_shared.hip):
// rows per batch tile for the loss layout, and the launch itself.
int shared_loss_batch_tile(const int* width, int layers);
int bf16_loss_batch_tile(const int* width, int layers);
void launch_shared_loss(const SharedForwardArgs& args, const SharedLossArgs& largs, int bt, hipStream_t stream);
void launch_shared_loss_bf16(const SharedForwardArgs& args, const SharedLossArgs& largs, int bt, hipStream_t stream);

#if defined(__HIPCC__)

// Maximum over each group of G lanes, in every lane of the group.
template <int G>
__device__ __forceinline__ float loss_group_max(float x) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) x = fmaxf(x, __shfl_xor(x, d, kWaveSize));
    return x;
}

// The sum of the losses of the wave's rows [row0, row0 + rows) of the tile
// (rows a multiple of 64 / G), wave-uniform. `tile` is fp32 with a row stride
// of `stride` floats; tile row r is batch row b0 + r.
template <int G>
__device__ __forceinline__ float loss_wave_rows(const float* tile, int stride, int row0, int rows, int b0, int B, int D,
                                                const SharedLossArgs& la, int lane) {
    constexpr int kRowsPerPass = kWaveSize / G;
    const int gl = lane & (G - 1), group = lane / G;
    float acc = 0.0f;
    for (int r = 0; r < rows; r += kRowsPerPass) {
        const int row = row0 + r + group;
        const int b = b0 + row;
        const int bc = min(b, B - 1);  // rows past B read row B - 1 and are dropped
        const float* v = tile + row * stride;
        float row_loss;
        if (la.kind == kLossMse) {
            const float* yr = la.y_mse + (long)bc * D;
            float s = 0.0f;
            for (int c = gl; c < D; c += G) {
                const float d = v[c] - yr[c];
                s = fmaf(d, d, s);
            }
            row_loss = group_sum<G>(s);
        } else {
            float mx = -INFINITY;
            for (int c = gl; c < D; c += G) mx = fmaxf(mx, v[c]);
            mx = loss_group_max<G>(mx);
            float s = 0.0f;
            for (int c = gl; c < D; c += G) s += expf(v[c] - mx);
            s = group_sum<G>(s);
            const long long t = la.y_ce[bc];
            const bool inside = t >= 0 && t < D;
            const float vt = v[inside ? (int)t : 0];
            row_loss = inside ? (logf(s) + mx) - vt : (t == kLossIgnoreIndex ? 0.0f : NAN);
        }
        acc += b < B ? row_loss : 0.0f;  // the row's loss is in its group's last lane
    }
    const int ai = __builtin_bit_cast(int, acc);
    if constexpr (G == 64) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 63));
    } else {
        const float g0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 15));
        const float g1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 31));
        const float g2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 47));
        const float g3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 63));
        return ((g0 + g1) + g2) + g3;
    }
}

// The whole phase, entered by all 256 threads after the barrier that follows
// the last layer's stores. `tile` [BT][stride] is that layer's fp32 output;
// `red` is 8 words of LDS outside the tile (the last layer's input buffer,
// dead by now). Writes loss[m * tiles + tile_index].
template <int BT>
__device__ __forceinline__ void shared_loss_phase(const float* tile, int stride, float* red, int m, int tile_index,
                                                  const SharedForwardArgs& args, const SharedLossArgs& la) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = args.B, D = args.width[args.layers], b0 = tile_index * BT;
    constexpr int kRows = BT / 4;  // per wave: 4, 8 or 16, a multiple of the rows per pass
    const float wave_sum = la.group == 16 ? loss_wave_rows<16>(tile, stride, wave * kRows, kRows, b0, B, D, la, lane)
                                          : loss_wave_rows<64>(tile, stride, wave * kRows, kRows, b0, B, D, la, lane);
    int kept = 0;  // this wave's share of the targets that are not ignored
    if (la.kind == kLossCrossEntropy) {
        for (int i0 = 0; i0 < B; i0 += 256) {
            const int i = i0 + tid;
            const bool keep = i < B && la.y_ce[min(i, B - 1)] != kLossIgnoreIndex;
            kept += __popcll(__ballot(keep));
        }
    }
    int* red_i = reinterpret_cast<int*>(red);
    if (lane == 0) {
        red[wave] = wave_sum;
        red_i[4 + wave] = kept;
    }
    __syncthreads();
    if (tid == 0) {
        const float sum = ((red[0] + red[1]) + red[2]) + red[3];
        const float divisor = la.kind == kLossMse ? (float)B * (float)D
                                                  : (float)(((red_i[4] + red_i[5]) + red_i[6]) + red_i[7]);
        la.loss[(long)m * args.tiles + tile_index] = sum / divisor;
    }
}

#endif  // __HIPCC__

}  // namespace ea
