// K16: population-batched step of a recurrent policy stack, fp32 throughout:
// 1 to 4 weighted layers of which exactly ONE is an explicit-state RNN
// (tanh or ReLU) or LSTM (models/layers.py) and the others are K13's dense
// layers (nn.Linear + identity / tanh / ReLU). One launch computes, for
// every member m from its own flat vector params[m],
//
//   RNN   h' = act(W_ih · x + W_hh · h + (b_ih + b_hh))
//   LSTM  [i f g o] = W_ih · x + W_hh · h + (b_ih + b_hh)
//         c' = sigmoid(f) · c + sigmoid(i) · tanh(g),  h' = sigmoid(o) · tanh(c')
//
// with x the output of the layers before it, h' feeding the layers after it,
// and h' (and c') returned as the member's new state. This is models.Policy's
// per-step call for recurrent nets when the kernel is opted into.
//
// Layout of params[m], in named_parameters() order: a dense layer as in K13
// (W [N][K], b [N] if the stack has biases); the recurrent layer as
// W_ih [R][K], W_hh [R][H], b_ih [R], b_hh [R] with R = H (RNN) or R = 4H
// (LSTM, gate blocks i, f, g, o of H rows each).
//
// Work split (K13's, policy_forward.hip)
//   * A member is owned by ONE wave, four members share a 256-thread block,
//     and there is no block barrier: layers are separated by the wave-level
//     LDS fence.
//   * LDS is dynamic and sized from THIS stack (recurrent_lds_floats, used
//     by kernel and launcher alike): per wave two ping-pong activation
//     buffers of the widest layer input, rounded up to 4 floats, and one
//     buffer for h. 376 -> LSTM 64 -> 17 takes 13056 bytes a block where
//     K13's fixed buffers take 32768.
//   * Dense layers are K13's policy_layer. In the recurrent layer a group of
//     G lanes computes hidden unit j over the virtual row
//     [W_ih[j] | W_hh[j]] against [x | h] in LDS: two segments walked one
//     after the other, each with its own whole 16-byte words (lane g takes
//     words g, g + G, ...) and its own K % 4 tail (one element each to the
//     group's first lanes). G = 8, 16 or 64 is picked on the host from the
//     words of both segments together. An LSTM group computes the four gate
//     rows j, H + j, 2H + j, 3H + j at once in four accumulators, so every
//     x / h word is read from LDS once for four rows.
//   * DPP group sums follow (four for an LSTM); the group's last lane adds
//     b_ih + b_hh, applies the activation or the cell arithmetic (expf and
//     tanhf, not the fast variants), stores h' (and c') to global memory and
//     h' to the next LDS buffer, or to `out` when no layer follows. c is read
//     from and written to global memory only.
//   * Without a state (h undefined) the h segment is skipped and c is zero:
//     no state memory is read.
//
// Bounds: a 16-byte word is loaded only when it lies wholly inside its row,
// tail elements are loaded one by one, and units past H in the last pass
// recompute unit H - 1 and drop the result, so all lanes stay active for the
// DPP sums and every address stays inside the member.
//
// Determinism: out[m], new_h[m], new_c[m] depend bit for bit on params[m],
// obs[m], h[m], c[m] and the stack description only. The summation order is
// a fixed function of (K, H, G): the x segment, the h segment, the DPP tree,
// then the summed biases. No atomics; all stores are plain vector stores.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <tuple>

#include "check.h"
#include "policy_common.h"
#include "reduce.h"
#include "rollout_common.h"

namespace ea {

constexpr int kMembersPerBlock = 4;  // one wave each

struct RecurrentForwardArgs {
    const float* params;  // [n][L]
    const float* obs;     // [n][width[0]]
    const float* h;       // [n][H] or null: no state yet
    const float* c;       // [n][H] (LSTM with h given) or null
    float* out;           // [n][width[layers]]
    float* new_h;         // [n][H]
    float* new_c;         // [n][H] (LSTM) or null
    int n;
    long L;
    int layers;
    int has_bias;  // of the dense layers; the recurrent layer always has its two
    int width[kMaxLayers + 1];
    int act[kMaxLayers];
    int kind[kMaxLayers];
    int group[kMaxLayers];  // lanes per row (dense) or unit (recurrent) group: 8, 16 or 64
};

__host__ __device__ inline int round_up4(int v) { return (v + 3) & ~3; }

// Floats of one ping-pong activation buffer: the widest layer INPUT (every
// non-final output is the next layer's input), rounded up to whole words.
__host__ __device__ inline int recurrent_act_floats(const int* width, int layers) {
    int widest = 0;
    for (int l = 0; l < layers; ++l) widest = width[l] > widest ? width[l] : widest;
    return round_up4(widest);
}

// Floats of a wave's LDS: [ping][pong][h]; every part starts 16-byte aligned.
__host__ __device__ inline int recurrent_lds_floats(const int* width, int layers, int H) {
    return 2 * recurrent_act_floats(width, layers) + round_up4(H);
}

// acc += W_row[0:K) · x[0:K) for this lane's share of one segment: whole
// words gl, gl + G, ..., then the K % 4 tail. K13's policy_layer walk.
template <int G>
__device__ __forceinline__ float segment_dot(const float* __restrict__ Wr, const float* x, int K, int gl,
                                             float acc) {
    const int words = K >> 2;
    const int steps = (words + G - 1) / G;  // wave-uniform trip count
    const floatx4* x4 = reinterpret_cast<const floatx4*>(x);
#pragma unroll 4
    for (int s = 0; s < steps; ++s) {
        const int w = gl + s * G;
        const bool in = w < words;
        const int wc = in ? w : 0;  // steps >= 1 means words >= 1: word 0 is inside the row
        const floatx4_a4 wv = *reinterpret_cast<const floatx4_a4*>(Wr + 4 * wc);
        const floatx4 xv = x4[wc];
        float t = fmaf(wv.x, xv.x, acc);
        t = fmaf(wv.y, xv.y, t);
        t = fmaf(wv.z, xv.z, t);
        t = fmaf(wv.w, xv.w, t);
        acc = in ? t : acc;
    }
    if (gl < (K & 3)) {  // G >= 8 > 3: one trailing element per lane
        const int k = 4 * words + gl;
        acc = fmaf(Wr[k], x[k], acc);
    }
    return acc;
}

// The same walk over the four gate rows Wr, Wr + gate, Wr + 2 gate,
// Wr + 3 gate (gate = H * K floats): each x word is read once.
template <int G>
__device__ __forceinline__ void segment_dot4(const float* __restrict__ Wr, long gate, const float* x, int K, int gl,
                                             float (&acc)[4]) {
    const int words = K >> 2;
    const int steps = (words + G - 1) / G;
    const floatx4* x4 = reinterpret_cast<const floatx4*>(x);
#pragma unroll 2
    for (int s = 0; s < steps; ++s) {
        const int w = gl + s * G;
        const bool in = w < words;
        const int wc = in ? w : 0;
        const floatx4 xv = x4[wc];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const floatx4_a4 wv = *reinterpret_cast<const floatx4_a4*>(Wr + q * gate + 4 * wc);
            float t = fmaf(wv.x, xv.x, acc[q]);
            t = fmaf(wv.y, xv.y, t);
            t = fmaf(wv.z, xv.z, t);
            t = fmaf(wv.w, xv.w, t);
            acc[q] = in ? t : acc[q];
        }
    }
    if (gl < (K & 3)) {
        const int k = 4 * words + gl;
        const float xk = x[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fmaf(Wr[q * gate + k], xk, acc[q]);
    }
}

__device__ __forceinline__ float sigmoid_exact(float v) { return 1.0f / (1.0f + expf(-v)); }

// What a recurrent layer of one member reads and writes. p points at W_ih.
struct RecurrentLayerIo {
    const float* p;
    const float* x;      // LDS, K floats
    const float* hprev;  // LDS, H floats, or null: no state yet
    const float* c;      // global row, or null
    float* y;            // LDS for the next layer, or the global out row when this is the last
    float* new_h;        // global row
    float* new_c;        // global row (LSTM)
};

template <int G>
__device__ __forceinline__ void rnn_layer(const RecurrentLayerIo& io, int K, int H, int act, int lane) {
    constexpr int kUnitsPerPass = kWaveSize / G;
    const int gl = lane & (G - 1);
    const int group = lane / G;
    const float* W_ih = io.p;
    const float* W_hh = W_ih + (long)H * K;
    const float* b_ih = W_hh + (long)H * H;
    const float* b_hh = b_ih + H;
    for (int unit0 = 0; unit0 < H; unit0 += kUnitsPerPass) {
        const int unit = unit0 + group;
        const int u = min(unit, H - 1);
        float acc = segment_dot<G>(W_ih + (long)u * K, io.x, K, gl, 0.0f);
        if (io.hprev != nullptr) acc = segment_dot<G>(W_hh + (long)u * H, io.hprev, H, gl, acc);
        acc = group_sum<G>(acc);
        if (gl == G - 1 && unit < H) {
            const float v = policy_activation(acc + (b_ih[unit] + b_hh[unit]), act);
            io.new_h[unit] = v;
            io.y[unit] = v;
        }
    }
}

template <int G>
__device__ __forceinline__ void lstm_layer(const RecurrentLayerIo& io, int K, int H, int lane) {
    constexpr int kUnitsPerPass = kWaveSize / G;
    const int gl = lane & (G - 1);
    const int group = lane / G;
    const float* W_ih = io.p;
    const float* W_hh = W_ih + 4L * H * K;
    const float* b_ih = W_hh + 4L * H * H;
    const float* b_hh = b_ih + 4 * H;
    for (int unit0 = 0; unit0 < H; unit0 += kUnitsPerPass) {
        const int unit = unit0 + group;
        const int u = min(unit, H - 1);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        segment_dot4<G>(W_ih + (long)u * K, (long)H * K, io.x, K, gl, acc);
        if (io.hprev != nullptr) segment_dot4<G>(W_hh + (long)u * H, (long)H * H, io.hprev, H, gl, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = group_sum<G>(acc[q]);
        if (gl == G - 1 && unit < H) {
            const float gi = sigmoid_exact(acc[0] + (b_ih[unit] + b_hh[unit]));
            const float gf = sigmoid_exact(acc[1] + (b_ih[H + unit] + b_hh[H + unit]));
            const float gg = tanhf(acc[2] + (b_ih[2 * H + unit] + b_hh[2 * H + unit]));
            const float go = sigmoid_exact(acc[3] + (b_ih[3 * H + unit] + b_hh[3 * H + unit]));
            const float c_old = io.c != nullptr ? io.c[unit] : 0.0f;
            const float c_new = gf * c_old + gi * gg;
            const float v = go * tanhf(c_new);
            io.new_c[unit] = c_new;
            io.new_h[unit] = v;
            io.y[unit] = v;
        }
    }
}

__global__ __launch_bounds__(kMembersPerBlock* kWaveSize) void population_recurrent_forward_kernel(
    RecurrentForwardArgs args) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kWaveSize - 1);
    const int wave = threadIdx.x / kWaveSize;
    const int m = blockIdx.x * kMembersPerBlock + wave;
    if (m >= args.n) return;  // wave-uniform; the kernel has no block barrier

    int H = 0;
    for (int l = 0; l < args.layers; ++l)
        if (args.kind[l] != kKindDense) H = args.width[l + 1];
    const int act_floats = recurrent_act_floats(args.width, args.layers);
    float* cur = lds + wave * recurrent_lds_floats(args.width, args.layers, H);
    float* nxt = cur + act_floats;
    float* hbuf = nxt + act_floats;

    const int D0 = args.width[0];
    const float* obs = args.obs + (long)m * D0;
    for (int k = lane; k < D0; k += kWaveSize) cur[k] = obs[k];
    if (args.h != nullptr) {
        const float* h = args.h + (long)m * H;
        for (int k = lane; k < H; k += kWaveSize) hbuf[k] = h[k];
    }
    wave_lds_fence();

    const float* p = args.params + (long)m * args.L;
    for (int l = 0; l < args.layers; ++l) {
        const int K = args.width[l], N = args.width[l + 1];
        const bool last = l + 1 == args.layers;
        const int G = args.group[l];
        const int kind = args.kind[l];
        if (kind == kKindDense) {
            const float* W = p;
            p += (long)N * K;
            const float* b = nullptr;
            if (args.has_bias) {
                b = p;
                p += N;
            }
            float* y = last ? args.out + (long)m * N : nxt;
            if (G == 8) {
                policy_layer<8>(W, b, cur, y, K, N, args.act[l], lane);
            } else if (G == 16) {
                policy_layer<16>(W, b, cur, y, K, N, args.act[l], lane);
            } else {
                policy_layer<64>(W, b, cur, y, K, N, args.act[l], lane);
            }
        } else {
            RecurrentLayerIo io;
            io.p = p;
            io.x = cur;
            io.hprev = args.h != nullptr ? hbuf : nullptr;
            io.c = args.c != nullptr ? args.c + (long)m * N : nullptr;
            io.y = last ? args.out + (long)m * N : nxt;
            io.new_h = args.new_h + (long)m * N;
            io.new_c = args.new_c != nullptr ? args.new_c + (long)m * N : nullptr;
            if (kind == kKindRnn) {
                p += (long)N * K + (long)N * N + 2 * N;
                if (G == 8) {
                    rnn_layer<8>(io, K, N, args.act[l], lane);
                } else if (G == 16) {
                    rnn_layer<16>(io, K, N, args.act[l], lane);
                } else {
                    rnn_layer<64>(io, K, N, args.act[l], lane);
                }
            } else {
                p += 4 * ((long)N * K + (long)N * N + 2 * N);
                if (G == 8) {
                    lstm_layer<8>(io, K, N, lane);
                } else if (G == 16) {
                    lstm_layer<16>(io, K, N, lane);
                } else {
                    lstm_layer<64>(io, K, N, lane);
                }
            }
        }
        if (!last) {
            wave_lds_fence();
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
    }
}

// Lanes per unit group of a recurrent layer: K13's rule (policy_group_width)
// on the words of the x and the h segment together.
static int recurrent_group_width(int K, int H) { return policy_group_width(4 * (K / 4 + H / 4)); }

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> population_recurrent_forward(
    torch::Tensor params, torch::Tensor obs, c10::optional<torch::Tensor> h, c10::optional<torch::Tensor> c,
    std::vector<int64_t> kinds, std::vector<int64_t> widths, std::vector<int64_t> activations, bool has_bias) {
    check_primary(params, "params", 2);
    TORCH_CHECK(params.scalar_type() == torch::kFloat32, "params must be float32, got ", params.scalar_type());
    RecurrentForwardArgs args{};
    int recurrent = 0;
    const int64_t expected =
        check_recurrent_stack(kinds, widths, activations, has_bias, args.width, args.act, args.kind, &recurrent);
    const int64_t layers = (int64_t)widths.size() - 1;
    const int64_t H = widths[recurrent + 1];
    const bool lstm = args.kind[recurrent] == kKindLstm;
    for (int64_t i = 0; i < layers; ++i)
        args.group[i] = i == recurrent ? recurrent_group_width(args.width[i], (int)H) : policy_group_width(args.width[i]);
    const int64_t n = params.size(0), L = params.size(1);
    TORCH_CHECK(L == expected, "params must hold ", expected, " values per member for this stack, got L = ", L);
    TORCH_CHECK(n <= INT_MAX / kMaxWidth, "params: too many members (", n, ")");
    check_operand(obs, "obs", params, n * widths[0]);
    const bool has_h = h.has_value() && h->defined();
    const bool has_c = c.has_value() && c->defined();
    if (has_h) {
        TORCH_CHECK(h->dim() == 2 && h->size(0) == n && h->size(1) == H, "h must be [", n, ", ", H, "], got ",
                    h->sizes());
        check_operand(*h, "h", params, n * H);
    }
    TORCH_CHECK(has_c == (lstm && has_h), "c must be given exactly when the recurrent layer is an LSTM and h is given");
    if (has_c) {
        TORCH_CHECK(c->dim() == 2 && c->size(0) == n && c->size(1) == H, "c must be [", n, ", ", H, "], got ",
                    c->sizes());
        check_operand(*c, "c", params, n * H);
    }

    torch::Tensor out = torch::empty({n, widths[layers]}, params.options());
    torch::Tensor new_h = torch::empty({n, H}, params.options());
    torch::Tensor new_c = lstm ? torch::empty({n, H}, params.options()) : torch::empty({0}, params.options());
    if (n == 0) return {out, new_h, new_c};
    args.params = params.data_ptr<float>();
    args.obs = obs.data_ptr<float>();
    args.h = has_h ? h->data_ptr<float>() : nullptr;
    args.c = has_c ? c->data_ptr<float>() : nullptr;
    args.out = out.data_ptr<float>();
    args.new_h = new_h.data_ptr<float>();
    args.new_c = lstm ? new_c.data_ptr<float>() : nullptr;
    args.n = (int)n;
    args.L = (long)L;
    args.layers = (int)layers;
    args.has_bias = has_bias ? 1 : 0;
    // at most 4 * (2 * 1024 + 1024) * 4 = 48 KB: under the 64 KB a launch gets without asking
    const size_t lds_bytes =
        (size_t)kMembersPerBlock * recurrent_lds_floats(args.width, args.layers, (int)H) * sizeof(float);
    const int blocks = (int)((n + kMembersPerBlock - 1) / kMembersPerBlock);
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(population_recurrent_forward_kernel, dim3(blocks), dim3(kMembersPerBlock * kWaveSize),
                       lds_bytes, stream, args);
    return {out, new_h, new_c};
}

}  // namespace ea
