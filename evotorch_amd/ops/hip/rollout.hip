// K10+K11 fused: whole-generation rollout of a population of policies
// through the synthetic vectorized environment, one kernel launch per
// generation (SURVEY.md §3.4 — the VecGymNE hot loop, collapsed).
//
// This file holds the dispatcher `rollout_linear` — with `prepare_rollout`,
// `select_rollout_kernel` and `launch_selected` the one place that
// validates, fills RolloutArgs, picks a kernel and sums the obs-stat
// partials — its early-terminating sibling `rollout_terminating`, the
// kernel-name query, and v6, the general kernel (any geometry, linear
// or MLP policy). The Humanoid-geometry kernels live in rollout_v7.hip (linear,
// MFMA) and rollout_m7.hip (MLP-64); shared helpers in rollout_common.h.
//
// Policies: linear (obs -> act) or one-hidden-layer tanh MLP
// (obs -> H -> act; H=64 is the reference paper's brax-humanoid config).
//
// MI355X design (v6): one workgroup rolls out kMembers (2 where they fit)
// population members for the entire T-step episode with policy weights
// AND the shared environment matrices resident in LDS — the inner loop
// never touches global memory. Multi-member blocks exist because one
// member's per-step work underfills a 512-thread block; gfx950 allows the
// required LDS (sharedMemPerBlock = 160 KB, probed; ~75 KB for 2 linear
// members, ~146 KB for 2 MLP-64 members).
//
// All inner products run on `v_dot2_f32_bf16` (2 bf16 MACs/instruction,
// fp32 accumulate). LDS access patterns:
//   * group-reduced dots (policy layers, dynamics factor V): row-major
//     [out][len]; 8-lane groups read consecutive bf16x2 — conflict-free,
//     with a 3-level shuffle reduction (64-lane trees serialized 6
//     dependent shuffles; measured 10:1 SQ_WAIT:SQ_BUSY).
//   * per-thread dots (U, D2): PAIR-INTERLEAVED COLUMN-MAJOR [K/2][O]
//     bf16x2 — one 4 B read per dot2 at lane-consecutive addresses.
// Observation-normalization statistics (sum, sumsq) accumulate per-thread
// in registers; at the end every (block, member) writes its own slice
// with plain stores and the dispatcher sums the slices with one torch
// reduction — run-to-run deterministic (K11; they become a single RCCL
// all-reduce across ranks — SURVEY.md §2.8 P5).
//
// Environment spec (must match the eager reference in
// evotorch_amd/neuroevolution/synthetic_env.py::rollout_eager, which
// quantizes the same operands to bf16):
//   obs_n = bf16((obs − mean) · inv_std)
//   hid   = bf16(tanh(W1·obs_n + b1))            (MLP mode only)
//   a     = clip(W2·hid + b2, −1, 1)   |  clip(W·obs_n + b, −1, 1)
//   h     = bf16(V·obs)
//   o'    = tanh(Σ_i U_T[i]·h[i] + Σ_m D2_T[m]·a[m] + c)
//   r     = wr·o' + alive_bonus − act_cost·‖a‖²/A
//   o₀    = 0.1·philox_normal(member);  fitness = Σ_t r_t
// Terminating variant: a member is done after the step whose
// bf16(o'[health_index]) is outside [healthy_lo, healthy_hi]; Σ_t then
// runs over its len steps, and len goes to steps_out.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdlib>
#include <string>

#include "philox.h"
#include "reduce.h"
#include "rollout_common.h"

namespace ea {

// runtime member-index -> pointer select WITHOUT a runtime-indexed array
// (which would demote to scratch memory — common-mistake #20); for
// kMembers<=2 this folds to a single v_cndmask per operand.
template <typename T>
__device__ __forceinline__ T* sel2(int m, T* p0, T* p1) {
    return m == 0 ? p0 : p1;
}

// Dynamic-LDS layout of the v6 kernel (byte offsets): the one statement of
// it, for the kernel's carve-up and the launcher's footprint alike.
struct V6Layout {
    int A_PAD, R_PAD;                                       // even, with at least one zero pad element
    size_t V, U_pair, D2_pair, c, wr, mean, istd, scratch;  // shared environment
    size_t member0, member_stride;                          // member m's region starts at member0 + m * member_stride
    size_t W1, b1, W2, b2, hid, obs, obsn, h, act;          // within a member's region
    size_t flags;                                           // int [members] alive flags (terminating kernel only)
    size_t bytes;
};

__host__ __device__ inline V6Layout v6_layout(int O, int A, int R, int H, int members) {
    V6Layout l;
    l.A_PAD = (A + 2) & ~1;
    l.R_PAD = (R + 2) & ~1;
    const size_t w1_rows = (H > 0) ? H : A;
    size_t at = 0;
    const auto take = [&at](size_t n_bytes) {
        const size_t offset = at;
        at += n_bytes;
        return offset;
    };
    l.V = take((size_t)R * O * 2);                  // bf16 [R][O]
    l.U_pair = take((size_t)l.R_PAD / 2 * O * 4);   // bf16x2 [R_PAD/2][O]
    l.D2_pair = take((size_t)l.A_PAD / 2 * O * 4);  // bf16x2 [A_PAD/2][O]
    l.c = take((size_t)O * 4);                      // float [O]
    l.wr = take((size_t)O * 4);                     // float [O]
    l.mean = take((size_t)O * 4);                   // float [O]
    l.istd = take((size_t)O * 4);                   // float [O]
    l.scratch = take(16 * 4);                       // float [16] block-reduction scratch
    l.member0 = at;
    at = 0;
    l.W1 = take(w1_rows * O * 2);                   // bf16, linear: [A][O]; MLP: [H][O]
    l.b1 = take(w1_rows * 4);                       // float, linear: [A]; MLP: [H]
    l.W2 = take(H > 0 ? (size_t)A * H * 2 : 0);     // bf16 [A][H], MLP only
    l.b2 = take(H > 0 ? (size_t)A * 4 : 0);         // float [A], MLP only
    l.hid = take(H > 0 ? (size_t)H * 2 : 0);        // bf16 [H], MLP only
    l.obs = take((size_t)O * 2);                    // bf16 [O]
    l.obsn = take((size_t)O * 2);                   // bf16 [O]
    l.h = take((size_t)l.R_PAD * 2);                // bf16 [R_PAD]
    l.act = take((size_t)l.A_PAD * 2);              // bf16 [A_PAD]
    l.member_stride = at;
    // 64 B of tail slack the launcher has always requested; kept so the
    // footprint and the two-member threshold stay where they were. The
    // terminating kernel keeps its alive flags there (every region before
    // it is a multiple of 4 B: O and H are even).
    l.flags = l.member0 + (size_t)members * l.member_stride;
    l.bytes = l.flags + 64;
    return l;
}

// one group-reduced dot output: 8 lanes compute row·vec, lane 0 of the
// group applies the epilogue selected by `kind`
struct OutDesc {
    const __bf16* row;
    const __bf16* vec;
    __bf16* dst;
    const float* bias;   // null for kind 0
    int kind;            // 0 = plain store, 1 = action (bias+clip), 2 = hidden (bias+tanh)
    int member;
    bool valid;
};

// kTerm adds early episode termination (see the flag protocol at the step
// loop); everything it needs sits behind `if constexpr (kTerm)`, and a live
// member runs the same arithmetic sequence in both instantiations.
template <int kGroup, int kMembers, bool kTerm>
__global__ __launch_bounds__(512, 2) void rollout_linear_kernel(RolloutArgs args) {
    const int O = args.obs_dim, A = args.act_dim, R = args.rank, H = args.hidden;
    const int tid = threadIdx.x;
    const int base_member = blockIdx.x * kMembers;
    if (base_member >= args.n_members) return;
    const int live_members = min(kMembers, args.n_members - base_member);
    const long param_len = (H > 0) ? ((long)H * O + H + (long)A * H + A) : ((long)A * O + A);

    extern __shared__ unsigned char lds_raw[];
    const V6Layout lay = v6_layout(O, A, R, H, kMembers);
    const int A_PAD = lay.A_PAD, R_PAD = lay.R_PAD;
    // ---- shared environment ----
    __bf16* V_l = reinterpret_cast<__bf16*>(lds_raw + lay.V);
    bf16x2* U_pair = reinterpret_cast<bf16x2*>(lds_raw + lay.U_pair);
    bf16x2* D2_pair = reinterpret_cast<bf16x2*>(lds_raw + lay.D2_pair);
    float* c_l = reinterpret_cast<float*>(lds_raw + lay.c);
    float* wr_l = reinterpret_cast<float*>(lds_raw + lay.wr);
    float* mean_l = reinterpret_cast<float*>(lds_raw + lay.mean);
    float* istd_l = reinterpret_cast<float*>(lds_raw + lay.istd);
    float* scratch = reinterpret_cast<float*>(lds_raw + lay.scratch);
    // ---- per-member state (W2, b2, hid: MLP only) ----
    __bf16* W1_l[kMembers];
    float* b1_l[kMembers];
    __bf16* W2_l[kMembers];
    float* b2_l[kMembers];
    __bf16* hid_b[kMembers];
    __bf16* obs_b[kMembers];
    __bf16* obsn_b[kMembers];
    __bf16* h_b[kMembers];
    __bf16* act_b[kMembers];
#pragma unroll
    for (int m = 0; m < kMembers; ++m) {
        unsigned char* mine = lds_raw + lay.member0 + m * lay.member_stride;
        W1_l[m] = reinterpret_cast<__bf16*>(mine + lay.W1);
        b1_l[m] = reinterpret_cast<float*>(mine + lay.b1);
        W2_l[m] = reinterpret_cast<__bf16*>(mine + lay.W2);
        b2_l[m] = reinterpret_cast<float*>(mine + lay.b2);
        hid_b[m] = reinterpret_cast<__bf16*>(mine + lay.hid);
        obs_b[m] = reinterpret_cast<__bf16*>(mine + lay.obs);
        obsn_b[m] = reinterpret_cast<__bf16*>(mine + lay.obsn);
        h_b[m] = reinterpret_cast<__bf16*>(mine + lay.h);
        act_b[m] = reinterpret_cast<__bf16*>(mine + lay.act);
    }

    // ---- stage shared env ----
    {
        const EnvBlob env(args.env_blob, O, A, R);
        for (int i = tid; i < R * O; i += blockDim.x) V_l[i] = f2b(env.V[i]);
        for (int i = tid; i < (R_PAD / 2) * O; i += blockDim.x) {
            const int i2 = i / O, j = i % O;
            bf16x2 v2;
            v2.x = (2 * i2 < R) ? f2b(env.U_T[(2 * i2) * O + j]) : f2b(0.0f);
            v2.y = (2 * i2 + 1 < R) ? f2b(env.U_T[(2 * i2 + 1) * O + j]) : f2b(0.0f);
            U_pair[i2 * O + j] = v2;
        }
        for (int i = tid; i < (A_PAD / 2) * O; i += blockDim.x) {
            const int m2 = i / O, j = i % O;
            bf16x2 v2;
            v2.x = (2 * m2 < A) ? f2b(env.D2_T[(2 * m2) * O + j]) : f2b(0.0f);
            v2.y = (2 * m2 + 1 < A) ? f2b(env.D2_T[(2 * m2 + 1) * O + j]) : f2b(0.0f);
            D2_pair[m2 * O + j] = v2;
        }
        for (int j = tid; j < O; j += blockDim.x) {
            c_l[j] = env.c[j];
            wr_l[j] = env.wr[j];
            mean_l[j] = env.mean[j];
            istd_l[j] = 1.0f / env.std[j];
        }
    }
    // alive flags: 1 for a live slot, 0 for the empty slot of a half-live block
    [[maybe_unused]] int* alive_l = reinterpret_cast<int*>(lds_raw + lay.flags);
    if constexpr (kTerm) {
        if (tid < kMembers) alive_l[tid] = tid < live_members;
    }
    // ---- stage members: weights, pads, initial observations ----
#pragma unroll
    for (int m = 0; m < kMembers; ++m) {
        if (m >= live_members) break;
        const float* my_params = args.params + (long)(base_member + m) * param_len;
        if (H > 0) {
            for (int i = tid; i < H * O; i += blockDim.x) W1_l[m][i] = f2b(my_params[i]);
            for (int i = tid; i < H; i += blockDim.x) b1_l[m][i] = my_params[H * O + i];
            for (int i = tid; i < A * H; i += blockDim.x) W2_l[m][i] = f2b(my_params[H * O + H + i]);
            for (int i = tid; i < A; i += blockDim.x) b2_l[m][i] = my_params[H * O + H + A * H + i];
        } else {
            for (int i = tid; i < A * O; i += blockDim.x) W1_l[m][i] = f2b(my_params[i]);
            for (int i = tid; i < A; i += blockDim.x) b1_l[m][i] = my_params[A * O + i];
        }
        for (int i = tid; i < R_PAD; i += blockDim.x) h_b[m][i] = f2b(0.0f);
        for (int i = tid; i < A_PAD; i += blockDim.x) act_b[m][i] = f2b(0.0f);
        const unsigned long long gmember = (unsigned long long)(args.member_offset + base_member + m);
        const unsigned long long iseed = args.seed_ptr ? *args.seed_ptr : args.init_seed;
        for (int j4 = tid; j4 * 4 < O; j4 += blockDim.x) {
            float z[4];
            philox_normal4(iseed, (uint32_t)gmember, (uint64_t)j4, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j4 * 4 + u;
                if (j < O) obs_b[m][j] = f2b(0.1f * z[u]);
            }
        }
    }
    __syncthreads();

    const int lane = tid & (kWaveSize - 1);
    const int wave = tid / kWaveSize;
    const int group = lane / kGroup;
    const int glane = lane % kGroup;
    const int groups_per_block = (int)(blockDim.x / kGroup);
    const int groups_per_wave = kWaveSize / kGroup;
    const int my_group = wave * groups_per_wave + group;

    // ---- phase-A table: dots over obs-side vectors -------------------------
    // Per member: H hidden outputs (MLP) or A action outputs (linear),
    // followed by R dynamics-factor outputs. Up to 3 rounds (e.g. 2 MLP-64
    // members: 2*(64+16) = 160 outputs over 64 groups).
    constexpr int kRoundsA = 3;
    const int a_per_member = (H > 0 ? H : A) + R;
    const int n_outs_a = live_members * a_per_member;
    OutDesc descA[kRoundsA];
#pragma unroll
    for (int r = 0; r < kRoundsA; ++r) {
        const int out = my_group + r * groups_per_block;
        OutDesc d;
        d.valid = out < n_outs_a;
        const int safe_out = d.valid ? out : 0;
        const int m = safe_out / a_per_member;
        const int lo = safe_out % a_per_member;
        d.member = m;
        const int first_count = (H > 0 ? H : A);
        __bf16* w1_m = sel2(m, W1_l[0], W1_l[kMembers - 1]);
        float* b1_m = sel2(m, b1_l[0], b1_l[kMembers - 1]);
        __bf16* obs_m = sel2(m, obs_b[0], obs_b[kMembers - 1]);
        __bf16* obsn_m = sel2(m, obsn_b[0], obsn_b[kMembers - 1]);
        __bf16* henv_m = sel2(m, h_b[0], h_b[kMembers - 1]);
        if (lo < first_count) {
            d.row = w1_m + lo * O;
            d.vec = obsn_m;
            d.bias = b1_m + lo;
            if (H > 0) {
                __bf16* hid_m = sel2(m, hid_b[0], hid_b[kMembers - 1]);
                d.dst = hid_m + lo;
                d.kind = 2;
            } else {
                __bf16* act_m = sel2(m, act_b[0], act_b[kMembers - 1]);
                d.dst = act_m + lo;
                d.kind = 1;
            }
        } else {
            d.row = V_l + (lo - first_count) * O;
            d.vec = obs_m;
            d.bias = nullptr;
            d.dst = henv_m + (lo - first_count);
            d.kind = 0;
        }
        descA[r] = d;
    }
    // ---- phase-B table (MLP only): action dots over the hidden vector ------
    constexpr int kRoundsB = 1;
    OutDesc descB[kRoundsB];
#pragma unroll
    for (int r = 0; r < kRoundsB; ++r) {
        const int out = my_group + r * groups_per_block;
        OutDesc d;
        d.valid = (H > 0) && (out < live_members * A);
        const int safe_out = d.valid ? out : 0;
        const int m = safe_out / A;
        const int lo = safe_out % A;
        d.member = m;
        d.row = (H > 0) ? sel2(m, W2_l[0], W2_l[kMembers - 1]) + lo * H : nullptr;
        d.vec = (H > 0) ? sel2(m, hid_b[0], hid_b[kMembers - 1]) : nullptr;
        d.bias = (H > 0) ? sel2(m, b2_l[0], b2_l[kMembers - 1]) + lo : nullptr;
        d.dst = sel2(m, act_b[0], act_b[kMembers - 1]) + lo;
        d.kind = 1;
        descB[r] = d;
    }

    float fit_part[kMembers];
    float actsq_part[kMembers];
#pragma unroll
    for (int m = 0; m < kMembers; ++m) {
        fit_part[m] = 0.0f;
        actsq_part[m] = 0.0f;
    }
    float stat_sum[2] = {0.0f, 0.0f}, stat_sumsq[2] = {0.0f, 0.0f};
    // kTerm: this step's alive flags and the episode lengths, the same in
    // every thread of the block
    [[maybe_unused]] int alive_r[kMembers];
    [[maybe_unused]] int len_r[kMembers];
#pragma unroll
    for (int m = 0; m < kMembers; ++m) {
        alive_r[m] = 1;
        len_r[m] = 0;
    }
    // does member m take part in this step? (always, without termination)
    const auto member_on = [&alive_r](int m) -> bool {
        if constexpr (kTerm) return (m == 0 ? alive_r[0] : alive_r[kMembers - 1]) != 0;
        return true;
    };

    // initial normalization (later steps fuse it into phase 2's epilogue)
    for (int j = tid; j < live_members * O; j += blockDim.x) {
        const int m = j / O, jo = j % O;
        __bf16* obs_m = sel2(m, obs_b[0], obs_b[kMembers - 1]);
        __bf16* obsn_m = sel2(m, obsn_b[0], obsn_b[kMembers - 1]);
        obsn_m[jo] = f2b((b2f(obs_m[jo]) - mean_l[jo]) * istd_l[jo]);
    }
    __syncthreads();

    // an output is worked on when its table entry is in use and (kTerm) its
    // member is still alive: a done member's dots, stores and action cost
    // are skipped. The test is uniform over the 8-lane group.
#define DESC_ON(d) ((d).valid && member_on((d).member))

    // group-dot worker: acc[r] = descs[r].row · descs[r].vec  (length
    // 2*n_pairs), reduced across the kGroup lanes of the group
#define GROUP_DOTS(descs, NR, n_pairs_expr, acc)                                              \
    {                                                                                         \
        const int np = (n_pairs_expr);                                                        \
        _Pragma("unroll") for (int r = 0; r < (NR); ++r) acc[r] = 0.0f;                       \
        _Pragma("unroll") for (int r = 0; r < (NR); ++r) {                                    \
            if (!DESC_ON(descs[r])) continue;                                                 \
            const __bf16* row = descs[r].row;                                                 \
            const __bf16* vec = descs[r].vec;                                                 \
            float a0 = 0.0f, a1 = 0.0f;                                                       \
            const int full_iters = np / kGroup;                                               \
            const int tail = np % kGroup;                                                     \
            for (int i = 0; i + 1 < full_iters; i += 2) {                                     \
                const int p0 = glane + i * kGroup;                                            \
                const int p1 = glane + (i + 1) * kGroup;                                      \
                a0 = __builtin_amdgcn_fdot2_f32_bf16(                                         \
                    *reinterpret_cast<const bf16x2*>(row + 2 * p0),                           \
                    *reinterpret_cast<const bf16x2*>(vec + 2 * p0), a0, false);               \
                a1 = __builtin_amdgcn_fdot2_f32_bf16(                                         \
                    *reinterpret_cast<const bf16x2*>(row + 2 * p1),                           \
                    *reinterpret_cast<const bf16x2*>(vec + 2 * p1), a1, false);               \
            }                                                                                 \
            if (full_iters & 1) {                                                             \
                const int p0 = glane + (full_iters - 1) * kGroup;                             \
                a0 = __builtin_amdgcn_fdot2_f32_bf16(                                         \
                    *reinterpret_cast<const bf16x2*>(row + 2 * p0),                           \
                    *reinterpret_cast<const bf16x2*>(vec + 2 * p0), a0, false);               \
            }                                                                                 \
            if (tail && glane < tail) {                                                       \
                const int p0 = glane + full_iters * kGroup;                                   \
                a1 = __builtin_amdgcn_fdot2_f32_bf16(                                         \
                    *reinterpret_cast<const bf16x2*>(row + 2 * p0),                           \
                    *reinterpret_cast<const bf16x2*>(vec + 2 * p0), a1, false);               \
            }                                                                                 \
            acc[r] = a0 + a1;                                                                 \
        }                                                                                     \
        _Pragma("unroll") for (int r = 0; r < (NR); ++r) {                                    \
            /* VALU DPP group reduce; group sums land in glane == kGroup-1 */                 \
            if (DESC_ON(descs[r])) acc[r] = group8_sum_dpp(acc[r]);                           \
        }                                                                                     \
    }

#define DOT_EPILOGUE(descs, NR, acc)                                                          \
    if (glane == kGroup - 1) {                                                                \
        _Pragma("unroll") for (int r = 0; r < (NR); ++r) {                                    \
            if (!DESC_ON(descs[r])) continue;                                                 \
            if (descs[r].kind == 1) {                                                         \
                const float a = fminf(fmaxf(acc[r] + *descs[r].bias, -1.0f), 1.0f);           \
                *descs[r].dst = f2b(a);                                                       \
                _Pragma("unroll") for (int m = 0; m < kMembers; ++m) {                        \
                    if (descs[r].member == m) actsq_part[m] = fmaf(a, a, actsq_part[m]);      \
                }                                                                             \
            } else if (descs[r].kind == 2) {                                                  \
                *descs[r].dst = f2b(tanh_fast(acc[r] + *descs[r].bias));                      \
            } else {                                                                          \
                *descs[r].dst = f2b(acc[r]);                                                  \
            }                                                                                 \
        }                                                                                     \
    }

    // Termination (kTerm). alive_l[m] in LDS is cleared in the dynamics phase
    // by the one thread that owns (m, health_index); every thread copies the
    // flags into registers at the top of the next step. Those reads come
    // after the end-of-step barrier and before the phase-A barrier, the next
    // write comes after it: no race and no extra barrier. All threads read
    // the same flags, so the early exit is block-uniform.
    for (int t = 0; t < args.steps; ++t) {
        if constexpr (kTerm) {
            int any_alive = 0;
#pragma unroll
            for (int m = 0; m < kMembers; ++m) {
                alive_r[m] = alive_l[m];
                len_r[m] += alive_r[m];
                any_alive |= alive_r[m];
            }
            if (!any_alive) break;
        }
        // ---- phase A: hidden (or action) + dynamics-factor dots ----
        float accA[kRoundsA];
        GROUP_DOTS(descA, kRoundsA, O / 2, accA);
        DOT_EPILOGUE(descA, kRoundsA, accA);
        __syncthreads();

        // ---- phase B (MLP only): action dots over the hidden vector ----
        if (H > 0) {
            float accB[kRoundsB];
            GROUP_DOTS(descB, kRoundsB, H / 2, accB);
            DOT_EPILOGUE(descB, kRoundsB, accB);
            __syncthreads();
        }

        // ---- dynamics phase: per-thread dims, norm fused in epilogue ----
        for (int j = tid; j < live_members * O; j += blockDim.x) {
            const int m = j / O, jo = j % O;
            if (!member_on(m)) continue;  // a done member's sums and observation stay as they are
            float uacc = c_l[jo], dacc = 0.0f;
            const __bf16* hv = sel2(m, h_b[0], h_b[kMembers - 1]);
            const __bf16* av = sel2(m, act_b[0], act_b[kMembers - 1]);
#pragma unroll
            for (int p = 0; p < R_PAD / 2; ++p) {
                uacc = __builtin_amdgcn_fdot2_f32_bf16(
                    U_pair[p * O + jo], *reinterpret_cast<const bf16x2*>(hv + 2 * p), uacc, false);
            }
#pragma unroll
            for (int p = 0; p < A_PAD / 2; ++p) {
                dacc = __builtin_amdgcn_fdot2_f32_bf16(
                    D2_pair[p * O + jo], *reinterpret_cast<const bf16x2*>(av + 2 * p), dacc, false);
            }
            const float o_new = tanh_fast(uacc + dacc);
#pragma unroll
            for (int mm = 0; mm < kMembers; ++mm) {
                if (m == mm) fit_part[mm] = fmaf(wr_l[jo], o_new, fit_part[mm]);
            }
            const int slot = j >= (int)blockDim.x;
            stat_sum[slot] += o_new;
            stat_sumsq[slot] = fmaf(o_new, o_new, stat_sumsq[slot]);
            const __bf16 ob = f2b(o_new);
            __bf16* obs_m = sel2(m, obs_b[0], obs_b[kMembers - 1]);
            __bf16* obsn_m = sel2(m, obsn_b[0], obsn_b[kMembers - 1]);
            obs_m[jo] = ob;
            obsn_m[jo] = f2b((b2f(ob) - mean_l[jo]) * istd_l[jo]);
            if constexpr (kTerm) {
                // done after this step: the bf16 value the policy would see
                // next is outside the healthy range (a NaN is outside)
                const float health = b2f(ob);
                if (jo == args.health_index && !(args.healthy_lo <= health && health <= args.healthy_hi)) alive_l[m] = 0;
            }
        }
        __syncthreads();
    }

#undef GROUP_DOTS
#undef DOT_EPILOGUE
#undef DESC_ON

    // ---- wrap-up: per-member fitness reductions + obs-stat slices ----
#pragma unroll
    for (int m = 0; m < kMembers; ++m) {
        if (m >= live_members) break;
        const float total = block_reduce_sum<false>(fit_part[m], scratch);
        __syncthreads();
        const float act_total = block_reduce_sum<false>(actsq_part[m], scratch);
        __syncthreads();
        // the alive bonus is paid per step survived
        const int steps_m = kTerm ? len_r[m] : args.steps;
        if (tid == 0) {
            args.fitness_out[base_member + m] =
                total + args.alive_bonus * steps_m - args.act_cost * act_total / (float)A;
            if constexpr (kTerm) args.steps_out[base_member + m] = steps_m;
        }
    }
    // per-(block, member) stat slices: the j-loop visits each (m, jo) pair
    // exactly once, so plain stores are race-free and — unlike the float
    // atomicAdd they replace — run-to-run deterministic; the launcher sums
    // the partial slices with one torch reduction.
    for (int j = tid; j < live_members * O; j += blockDim.x) {
        const int slot = j >= (int)blockDim.x;
        const int m = j / O;
        const int jo = j % O;
        float* stats = args.obs_stats_out + ((int64_t)blockIdx.x * kMembers + m) * 2 * O;
        stats[jo] = stat_sum[slot];
        stats[O + jo] = stat_sumsq[slot];
    }
}


constexpr int kV6Threads = 512;

template <int kGroup, int kMembers, bool kTerm>
static void launch_rollout_v6(const RolloutArgs& args, int n_blocks, size_t lds_bytes, hipStream_t stream) {
    static bool attr_set = false;
    if (!attr_set && lds_bytes > 64 * 1024) {
        allow_max_dynamic_lds(reinterpret_cast<const void*>(&rollout_linear_kernel<kGroup, kMembers, kTerm>));
        attr_set = true;
    }
    hipLaunchKernelGGL((rollout_linear_kernel<kGroup, kMembers, kTerm>), dim3(n_blocks), dim3(kV6Threads), lds_bytes,
                       stream, args);
}

// v6 members per block: two where they fit in LDS, else one. Checks the
// footprint and the capacities of the kernel's fixed-size tables.
static int v6_members_per_block(int O, int A, int R, int H) {
    const int members = (v6_layout(O, A, R, H, 2).bytes > 160 * 1024) ? 1 : 2;
    const size_t lds_bytes = v6_layout(O, A, R, H, members).bytes;
    TORCH_CHECK(lds_bytes <= 160 * 1024, "rollout LDS footprint too large: ", lds_bytes, " bytes");
    // phase-A round capacity: up to 3 rounds of (threads/8) outputs
    TORCH_CHECK(members * ((H > 0 ? H : A) + R) <= 3 * kV6Threads / 8, "policy too wide for the 3-round phase-A table");
    TORCH_CHECK(members * A <= kV6Threads / 8, "act_dim too large for the 1-round phase-B table");
    TORCH_CHECK(O * members <= 2 * kV6Threads, "obs_dim too large for the 2-slot stat accumulators");
    return members;
}

// The one kernel selection, for both entry points and the name query. v7
// (MFMA, linear) and m7 (MLP-64) serve the Humanoid geometry; v7 also
// terminates, m7 does not. v6 covers every other geometry and policy width,
// terminating MLP-64, and everything when EVOTORCH_AMD_ROLLOUT_V6 is set.
// Read on every call: tests change it within a process.
enum class RolloutKernel { v6, v7, m7 };

static RolloutKernel select_rollout_kernel(int64_t O, int64_t A, int64_t R, int64_t H, bool terminating) {
    const bool humanoid = R == 16 && O == 376 && A == 17 && !getenv("EVOTORCH_AMD_ROLLOUT_V6");
    if (humanoid && H == 0) return RolloutKernel::v7;
    if (humanoid && H == 64 && !terminating) return RolloutKernel::m7;
    return RolloutKernel::v6;
}

std::string rollout_kernel_name(int64_t obs_dim, int64_t act_dim, int64_t rank, int64_t policy_hidden,
                                bool terminating) {
    switch (select_rollout_kernel(obs_dim, act_dim, rank, policy_hidden, terminating)) {
        case RolloutKernel::v7: return "v7";
        case RolloutKernel::m7: return "m7";
        default: return "v6";
    }
}

// A validated rollout call: the checked operands turned into kernel
// arguments (all but obs_stats_out, which each entry point sizes for the
// kernel it picks) and the fitness tensor the kernel writes.
struct RolloutCall {
    RolloutArgs args;
    int n, O, A, R, H;
    torch::Tensor fitness;
};

static RolloutCall prepare_rollout(const torch::Tensor& params, const torch::Tensor& env_blob,
                                   const torch::Tensor& obs_stats_out, int64_t obs_dim, int64_t act_dim, int64_t rank,
                                   int64_t steps, double alive_bonus, double act_cost, int64_t init_seed,
                                   int64_t member_offset, int64_t policy_hidden,
                                   const c10::optional<torch::Tensor>& seed_buf) {
    const unsigned long long* seed_ptr = seed_buf.has_value() ? device_i64_scalar(*seed_buf, "seed_buf") : nullptr;
    check_primary(params, "params", 2);
    TORCH_CHECK(params.scalar_type() == at::ScalarType::Float, "params must be fp32");
    const int n = (int)params.size(0);
    const int O = (int)obs_dim, A = (int)act_dim, R = (int)rank, H = (int)policy_hidden;
    const int64_t expected_len = (H > 0) ? ((int64_t)H * O + H + (int64_t)A * H + A) : ((int64_t)A * O + A);
    TORCH_CHECK(params.size(1) == expected_len, "param length mismatch: got ", params.size(1), " expected ", expected_len);
    TORCH_CHECK(O % 2 == 0, "obs_dim must be even (bf16x2 packing)");
    TORCH_CHECK(H % 2 == 0, "policy_hidden must be even (bf16x2 packing)");
    TORCH_CHECK(steps >= 0, "steps must be non-negative, got ", steps);
    // the sum of the EnvBlob layout in rollout_common.h
    check_operand(env_blob, "env_blob", params, (2 * (int64_t)R + A + 4) * O);
    check_operand(obs_stats_out, "obs_stats_out", params, 2 * (int64_t)O);

    RolloutCall call;
    call.n = n; call.O = O; call.A = A; call.R = R; call.H = H;
    call.fitness = torch::empty({n}, params.options());
    RolloutArgs& args = call.args;
    args.params = params.data_ptr<float>();
    args.env_blob = env_blob.data_ptr<float>();
    args.fitness_out = call.fitness.data_ptr<float>();
    args.obs_stats_out = nullptr;
    args.n_members = n;
    args.member_offset = (long)member_offset;
    args.obs_dim = O; args.act_dim = A; args.rank = R; args.hidden = H;
    args.steps = (int)steps;
    args.alive_bonus = (float)alive_bonus;
    args.act_cost = (float)act_cost;
    args.init_seed = (unsigned long long)init_seed;
    args.seed_ptr = seed_ptr;
    args.health_index = 0;
    args.healthy_lo = args.healthy_hi = 0.0f;
    args.steps_out = nullptr;
    return call;
}

// Picks the kernel of a validated call, sizes the obs-stat partials for it,
// launches, and adds the summed partials to obs_stats_out.
template <bool kTerm>
static void launch_selected(RolloutCall& call, const torch::Tensor& params, torch::Tensor& obs_stats_out) {
    RolloutArgs& args = call.args;
    const int n = call.n, O = call.O, A = call.A, R = call.R, H = call.H;
    const RolloutKernel kernel = select_rollout_kernel(O, A, R, H, kTerm);
    const bool use_v7 = kernel == RolloutKernel::v7, use_m7 = kernel == RolloutKernel::m7;
    const int members = use_v7 ? kV7MembersPerBlock : use_m7 ? kM7MembersPerBlock : v6_members_per_block(O, A, R, H);
    const int n_blocks = (n + members - 1) / members;
    // obs-stat partials: one row per block (v7, m7) or per (block, member)
    // (v6). The shapes fix the order of the torch reduction below.
    const int64_t stat_rows = (use_v7 || use_m7) ? n_blocks : (int64_t)n_blocks * members;
    auto stat_partials = torch::zeros({stat_rows, 2 * (int64_t)O}, params.options());
    args.obs_stats_out = stat_partials.data_ptr<float>();

    auto stream = at::cuda::getCurrentCUDAStream();
    if (use_v7) {
        launch_rollout_v7(args, n, stream, kTerm);
    } else if (use_m7) {
        launch_rollout_m7(args, n, stream);
    } else if (members == 2) {
        launch_rollout_v6<8, 2, kTerm>(args, n_blocks, v6_layout(O, A, R, H, 2).bytes, stream);
    } else {
        launch_rollout_v6<8, 1, kTerm>(args, n_blocks, v6_layout(O, A, R, H, 1).bytes, stream);
    }
    obs_stats_out.add_(stat_partials.sum(0));
}

torch::Tensor rollout_linear(torch::Tensor params, torch::Tensor env_blob, torch::Tensor obs_stats_out,
                             int64_t obs_dim, int64_t act_dim, int64_t rank, int64_t steps, double alive_bonus,
                             double act_cost, int64_t init_seed, int64_t member_offset, int64_t policy_hidden,
                             c10::optional<torch::Tensor> seed_buf) {
    RolloutCall call = prepare_rollout(params, env_blob, obs_stats_out, obs_dim, act_dim, rank, steps, alive_bonus,
                                       act_cost, init_seed, member_offset, policy_hidden, seed_buf);
    launch_selected<false>(call, params, obs_stats_out);
    return call.fitness;
}

// rollout_linear with early episode termination: member m is done after the
// step whose bf16(o'[health_index]) leaves [healthy_lo, healthy_hi], and its
// length goes to steps_out[m]. The terminating v7 for the linear policy at
// the Humanoid geometry, the terminating v6 everywhere else (m7 does not
// terminate).
torch::Tensor rollout_terminating(torch::Tensor params, torch::Tensor env_blob, torch::Tensor obs_stats_out,
                                  torch::Tensor steps_out, int64_t obs_dim, int64_t act_dim, int64_t rank,
                                  int64_t steps, double alive_bonus, double act_cost, int64_t init_seed,
                                  int64_t member_offset, int64_t policy_hidden, int64_t health_index,
                                  double healthy_lo, double healthy_hi, c10::optional<torch::Tensor> seed_buf) {
    RolloutCall call = prepare_rollout(params, env_blob, obs_stats_out, obs_dim, act_dim, rank, steps, alive_bonus,
                                       act_cost, init_seed, member_offset, policy_hidden, seed_buf);
    RolloutArgs& args = call.args;
    const int n = call.n, O = call.O;
    check_operand_as(steps_out, "steps_out", params, at::ScalarType::Int, n);
    TORCH_CHECK(health_index >= 0 && health_index < O, "health_index must be in [0, ", O, "), got ", health_index);
    // written so that a NaN bound fails it too
    TORCH_CHECK(healthy_lo <= healthy_hi, "healthy range must satisfy lo <= hi, got (", healthy_lo, ", ", healthy_hi,
                ")");
    args.health_index = (int)health_index;
    args.healthy_lo = (float)healthy_lo;
    args.healthy_hi = (float)healthy_hi;
    args.steps_out = steps_out.data_ptr<int>();

    launch_selected<true>(call, params, obs_stats_out);
    return call.fitness;
}

}  // namespace ea
