// m7: MLP-64 rollout at the Humanoid geometry (K10+K11) — 2-wave TEAMS per
// member, W1 register-resident. This file holds the m7 kernel and its
// launcher only; the dispatcher is in rollout.hip, the shared helpers in
// rollout_common.h.
//
// v6 runs MLP members with 8-lane group dots + block barriers and
// measures ~10:1 WAIT:BUSY (36 ms/gen at the reference MLP-64 config).
// Here each member is owned by a PAIR of waves: wave half h of the pair
// holds hidden rows [32h, 32h+32) of W1 in REGISTERS (32 rows x 6
// columns per lane = 96 VGPRs — a full per-member W1 cannot fit one
// wave, but half can), the observation lives in 3 bf16x2 registers per
// lane, and the layer-2 weights sit k-sliced per lane (17 bf16 = 9
// VGPRs). Per step: 32 col-sliced hidden dots per wave (DPP-reduced),
// one LDS exchange of the quantized h1 halves, the 17 action dots
// k-sliced over lanes, and the v8-style per-lane-column dynamics update
// with [U;D2] k-pairs from LDS. Two block barriers per step; both
// members of a block run the same schedule, so barriers stay balanced.
// 2-member 4-wave blocks run TWO per CU so blocks cover each other's
// stalls (a 4-member 8-wave block per CU exposed the barrier chain,
// measured slower, and was dropped).
// Numerics contract identical to v6/rollout_eager (bf16 operands, fp32
// accumulation, quantize-then-normalize, tanh on hidden and output).
// Default for the MLP-64 flagship geometry (29.4 vs v6's 36.4 ms at
// T=1000 popsize 4000, 1.24x); EVOTORCH_AMD_ROLLOUT_V6 forces v6.

#include <hip/hip_runtime.h>

#include "philox.h"
#include "rollout_common.h"

namespace ea {

// Compile-time geometry and the dynamic-LDS layout (byte offsets), stated
// once for the kernel's carve-up and the launcher's footprint.
template <int O, int A, int H>
struct M7Layout {
    static constexpr int kM = 2;                         // members per block, 2 waves each
    static constexpr int OP = (O + 127) / 128 * 128;     // 384 padded cols
    static constexpr int R = 16;
    static constexpr int K = R + A;                      // 33 dynamics rows
    static constexpr int KQ = (K + 1) / 2;               // 17 k-pairs
    static constexpr int VS = OP + 8;
    static constexpr int US = OP + 8;

    static constexpr int v = 0;                          // bf16 [R][VS]
    static constexpr int ud = v + R * VS * 2;            // bf16x2 [KQ][US]
    static constexpr int mean = ud + KQ * US * 4;        // float [OP]
    static constexpr int istd = mean + OP * 4;           // float [OP]
    static constexpr int c = istd + OP * 4;              // float [OP]
    static constexpr int wr = c + OP * 4;                // float [OP]
    static constexpr int h1 = wr + OP * 4;               // bf16 [2][kM][H] hidden (step-parity banks)
    static constexpr int act = h1 + 2 * kM * H * 2;      // float [2][kM][A + 1] actions
    static constexpr int hx = act + 2 * kM * (A + 1) * 4;  // float [2][kM][16] dynamics exchange
    static constexpr int sstat = hx + 2 * kM * 16 * 4;   // float [2][kM][OP] end only
    static constexpr int bytes = sstat + 2 * kM * OP * 4;
    static_assert(bytes <= 160 * 1024, "m7 LDS footprint exceeds the 160 KB of a gfx950 workgroup");
    static_assert(ud % 4 == 0 && mean % 4 == 0 && act % 4 == 0, "misaligned LDS region");
};

template <int O, int A, int H>
__global__ __launch_bounds__((M7Layout<O, A, H>::kM * 128), 2) void rollout_m7_kernel(RolloutArgs args) {
    using L = M7Layout<O, A, H>;
    constexpr int kM = L::kM, OP = L::OP, R = L::R, K = L::K, KQ = L::KQ, VS = L::VS, US = L::US;
    constexpr int kThreads = kM * 128;           // 2 waves per member
    constexpr int kPairs = OP / 2 / 64;          // 3 bf16x2 col-pairs per lane
    constexpr int kCols = 2 * kPairs;            // 6 cols per lane
    constexpr int HH = H / 2;                    // hidden rows per wave (32)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int member_slot = wave >> 1;           // 0..kM-1 within the block
    const int half = wave & 1;                   // which half of W1 this wave owns
    const int member = blockIdx.x * kM + member_slot;
    const bool live = member < args.n_members;
    const int mem_clamped = live ? member : 0;

    extern __shared__ unsigned char ldsm[];
    __bf16* v_l = reinterpret_cast<__bf16*>(ldsm + L::v);
    bf16x2* ud_l = reinterpret_cast<bf16x2*>(ldsm + L::ud);
    float* mean_l = reinterpret_cast<float*>(ldsm + L::mean);
    float* istd_l = reinterpret_cast<float*>(ldsm + L::istd);
    float* c_l = reinterpret_cast<float*>(ldsm + L::c);
    float* wr_l = reinterpret_cast<float*>(ldsm + L::wr);
    __bf16* h1_l = reinterpret_cast<__bf16*>(ldsm + L::h1);
    float* act_l = reinterpret_cast<float*>(ldsm + L::act);
    float* hx_l = reinterpret_cast<float*>(ldsm + L::hx);
    float* sstat = reinterpret_cast<float*>(ldsm + L::sstat);

    const EnvBlob env(args.env_blob, O, A, R);
    const float* e_M = env.U_T;  // [U;D2]: the K dynamics rows (U_T and D2_T are adjacent)

    for (int j = tid; j < R * VS; j += kThreads) {
        const int r = j / VS, cc = j % VS;
        v_l[j] = (cc < O) ? f2b(env.V[(size_t)r * O + cc]) : f2b(0.0f);
    }
    for (int j = tid; j < KQ * US; j += kThreads) {
        const int q = j / US, cc = j % US;
        bf16x2 m;
        m.x = (cc < O) ? f2b(e_M[(size_t)(2 * q) * O + cc]) : f2b(0.0f);
        m.y = (cc < O && 2 * q + 1 < K) ? f2b(e_M[(size_t)(2 * q + 1) * O + cc]) : f2b(0.0f);
        ud_l[j] = m;
    }
    for (int j = tid; j < OP; j += kThreads) {
        const bool in = j < O;
        mean_l[j] = in ? env.mean[j] : 0.0f;
        istd_l[j] = in ? 1.0f / env.std[j] : 0.0f;
        c_l[j] = in ? env.c[j] : 0.0f;
        wr_l[j] = in ? env.wr[j] : 0.0f;
    }

    // ---- per-member weights ----
    // params layout (synthetic_env.py): W1[H][O] b1[H] W2[A][H] b2[A]
    const long plen = (long)H * O + H + (long)A * H + A;
    const float* P = args.params + (long)mem_clamped * plen;
    bf16x2 w1[HH][kPairs];  // my half's rows x my col slice
#pragma unroll
    for (int r = 0; r < HH; ++r) {
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
            // lane owns STRIDE-64 single columns (lane + 64*(2p+e)) — the
            // two columns sharing a bf16x2 are 64 apart. fdot2 only needs
            // the same pairing in both operands; adjacent-pair ownership
            // made every GEMM2 [U;D2] read stride-2 per lane (measured
            // 0.99 LDS conflict cycles per LDS instruction).
            const int cx = lane + 64 * (2 * p);
            const int cy = lane + 64 * (2 * p + 1);
            const long row = (long)(half * HH + r) * O;
            bf16x2 w;
            w.x = (cx < O) ? f2b(P[row + cx]) : f2b(0.0f);
            w.y = (cy < O) ? f2b(P[row + cy]) : f2b(0.0f);
            w1[r][p] = w;
        }
    }
    float b1[HH];
#pragma unroll
    for (int r = 0; r < HH; ++r)
        b1[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P[(long)H * O + half * HH + r])));
    // W2 k-sliced: lane l holds W2[a][l] for all a (h1 index = lane)
    __bf16 w2[A];
#pragma unroll
    for (int a = 0; a < A; ++a) w2[a] = (lane < H) ? f2b(P[(long)H * O + H + (long)a * H + lane]) : f2b(0.0f);
    float b2[A];
#pragma unroll
    for (int a = 0; a < A; ++a)
        b2[a] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P[(long)H * O + H + (long)A * H + a])));

    float ssum[kCols] = {}, ssq[kCols] = {};
    float fit_acc = 0.0f;
    float asq_total = 0.0f;
    __syncthreads();

    // ---- initial observation ----
    const unsigned long long iseed = args.seed_ptr ? *args.seed_ptr : args.init_seed;
    bf16x2 obs2[kPairs], obsn2[kPairs];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        bf16x2 o, onr;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int col = lane + 64 * (2 * p + e);
            float z[4];
            philox_normal4(iseed, (uint32_t)(args.member_offset + member), (uint64_t)(col >> 2), z);
            // quad element = col & 3 = lane & 3 (64 ≡ 0 mod 4): branchless
            const float z01 = (lane & 1) ? z[1] : z[0];
            const float z23 = (lane & 1) ? z[3] : z[2];
            const float zv = (lane & 2) ? z23 : z01;
            const __bf16 ob = (col < O) ? f2b(0.1f * zv) : f2b(0.0f);
            const float onf = (b2f(ob) - mean_l[col < OP ? col : 0]) * istd_l[col < OP ? col : 0];
            if (e == 0) { o.x = ob; onr.x = f2b(onf); } else { o.y = ob; onr.y = f2b(onf); }
        }
        obs2[p] = o;
        obsn2[p] = onr;
    }

    for (int t = 0; t < args.steps; ++t) {
        // step-parity banks let the NEXT step's phase-A writes start
        // without a loop-end barrier (2 barriers per step, not 3)
        __bf16* h1b = h1_l + (t & 1) * kM * H;
        float* actb = act_l + (t & 1) * kM * (A + 1);
        float* hxb = hx_l + (t & 1) * kM * 16;
        // ---- hidden half: 32 col-sliced dots, DPP-reduced, quantized to LDS ----
        {
            // fused dot+reduce per row: row r+1's dot2s issue underneath
            // row r's DPP chain, and no 32-deep accumulator array stays
            // live (the separated two-loop form held 32 extra VGPRs).
            // v_readlane scalarization measured as the dominant stall
            // (SALU round-trips); one cross-half shuffle puts the 64-lane
            // total in lane 31, which writes directly.
#pragma unroll
            for (int r = 0; r < HH; ++r) {
                float acc = 0.0f;
#pragma unroll
                for (int p = 0; p < kPairs; ++p) acc = __builtin_amdgcn_fdot2_f32_bf16(w1[r][p], obsn2[p], acc, false);
                float s = reduce32_dpp(acc);
                s += __shfl_xor(s, 32, 64);
                if (lane == 31)
                    h1b[member_slot * H + half * HH + r] = f2b(tanh_fast(s + b1[r]));
            }
        }
        // ---- dynamics h = V @ obs is independent of h1: same phase, no
        // extra barrier (published into the sstat-scratch h-exchange) ----
        {
            float* hx = hxb;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const int r = half * 8 + rr;
                float acc = 0.0f;
#pragma unroll
                for (int p = 0; p < kPairs; ++p) {
                    bf16x2 v;
                    v.x = v_l[r * VS + lane + 64 * (2 * p)];
                    v.y = v_l[r * VS + lane + 64 * (2 * p + 1)];
                    acc = __builtin_amdgcn_fdot2_f32_bf16(v, obs2[p], acc, false);
                }
                float s = reduce32_dpp(acc);
                s += __shfl_xor(s, 32, 64);
                if (lane == 31) hx[member_slot * 16 + half * 8 + rr] = s;
            }
        }
        __syncthreads();
        // ---- actions: h1 k-sliced per lane (h index = lane); the 17
        // reductions split across BOTH halves of the member's wave pair ----
        {
            const float h1v = (lane < H) ? b2f(h1b[member_slot * H + lane]) : 0.0f;
            constexpr int kA0 = (A + 1) / 2;  // half 0: a < kA0; half 1: the rest
#pragma unroll
            for (int a = 0; a < A; ++a) {
                if ((half == 0) != (a < kA0)) continue;
                float part = b2f(w2[a]) * h1v;
                float s = reduce32_dpp(part);
                s += __shfl_xor(s, 32, 64);
                if (lane == 31)
                    actb[member_slot * (A + 1) + a] = fminf(fmaxf(s + b2[a], -1.0f), 1.0f);
            }
        }
        __syncthreads();
        {
            bf16x2 hact2[KQ];
            const float* hx = hxb;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                float kv[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int k = 2 * q + e;
                    if (k >= K) { kv[e] = 0.0f; continue; }
                    kv[e] = (k < R) ? hx[member_slot * 16 + k] : actb[member_slot * (A + 1) + (k - R)];
                }
                bf16x2 hp;
                hp.x = f2b(kv[0]);
                hp.y = f2b(kv[1]);
                hact2[q] = hp;
            }
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                bf16x2 o, onr;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int col = lane + 64 * (2 * p + e);
                    const int j = 2 * p + e;
                    float acc = 0.0f;
#pragma unroll
                    for (int q = 0; q < KQ; ++q)
                        acc = __builtin_amdgcn_fdot2_f32_bf16(ud_l[(size_t)q * US + col], hact2[q], acc, false);
                    const float o_new = tanh_fast(acc + c_l[col]);
                    if (half == 0) {  // one wave of the pair owns fitness/stats
                        fit_acc = fmaf(wr_l[col], o_new, fit_acc);
                        ssum[j] += o_new;
                        ssq[j] = fmaf(o_new, o_new, ssq[j]);
                    }
                    const __bf16 ob = f2b(o_new);
                    const float onf = (b2f(ob) - mean_l[col]) * istd_l[col];
                    if (e == 0) { o.x = ob; onr.x = f2b(onf); } else { o.y = ob; onr.y = f2b(onf); }
                }
                obs2[p] = o;
                obsn2[p] = onr;
            }
            if (half == 0 && lane < A) {
                const float av = actb[member_slot * (A + 1) + lane];
                asq_total = fmaf(av, av, asq_total);
            }
        }
        // no loop-end barrier: the next step writes the OTHER parity bank
    }
    __syncthreads();

    // ---- fitness wrap-up (wave half 0 of each member) ----
    if (half == 0) {
        float f = reduce32_dpp(fit_acc);
        float total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f), 31)) +
                      __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f), 63));
        float aq = reduce32_dpp(asq_total);
        float aq_total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, aq), 31)) +
                         __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, aq), 63));
        if (lane == 0 && live)
            args.fitness_out[member] =
                total + args.alive_bonus * (float)args.steps - args.act_cost * aq_total / (float)A;
    }
    __syncthreads();
    // ---- block stat partial (sstat was scratch during the loop; rebuilt now) ----
    if (half == 0) {  // one writer per member slot (the stats-owning wave)
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int col = lane + 64 * (2 * p + e);
                if (col < OP) {
                    sstat[(size_t)member_slot * OP + col] = live ? ssum[2 * p + e] : 0.0f;
                    sstat[(size_t)(kM + member_slot) * OP + col] = live ? ssq[2 * p + e] : 0.0f;
                }
            }
        }
    }
    __syncthreads();
    float* stats = args.obs_stats_out + (int64_t)blockIdx.x * 2 * O;
    for (int col = tid; col < O; col += kThreads) {
        float s = 0.0f, q = 0.0f;
#pragma unroll
        for (int w = 0; w < kM; ++w) {
            s += sstat[(size_t)w * OP + col];
            q += sstat[(size_t)(kM + w) * OP + col];
        }
        stats[col] = s;
        stats[O + col] = q;
    }
}

void launch_rollout_m7(const RolloutArgs& args, int n, hipStream_t stream) {
    constexpr int O_T = 376, A_T = 17, H_T = 64;
    using L = M7Layout<O_T, A_T, H_T>;
    static_assert(L::kM == kM7MembersPerBlock, "the dispatcher sizes the stat partials by kM7MembersPerBlock");
    TORCH_CHECK(args.obs_dim == O_T && args.act_dim == A_T && args.rank == L::R && args.hidden == H_T,
                "rollout m7 is instantiated for the MLP-64 policy at the Humanoid geometry (obs 376, act 17, rank 16)");
    static bool attr_set = false;
    if (!attr_set) {
        allow_max_dynamic_lds(reinterpret_cast<const void*>(&rollout_m7_kernel<O_T, A_T, H_T>));
        attr_set = true;
    }
    const int blocks = (n + L::kM - 1) / L::kM;
    hipLaunchKernelGGL((rollout_m7_kernel<O_T, A_T, H_T>), dim3(blocks), dim3(L::kM * 128), L::bytes, stream, args);
}

}  // namespace ea
