// v7 rollout: MFMA whole-episode rollout for the LINEAR flagship policy
// (K10+K11). This file holds the v7 kernel and its
// launcher only; the dispatcher is in rollout.hip, the MLP-64 kernel in
// rollout_m7.hip, the shared helpers in rollout_common.h.
//
// Why v7 beats v6 (2 members/block, all-v_dot2): v6 is LDS-bound — every
// dot2 reads 8 B of LDS for 4 FLOPs (~220 KB LDS traffic per block-step).
// The env dynamics (V·o, Uᵀh + D2ᵀa) have SHARED matrices across the
// population, i.e. real GEMMs once many members sit in one block:
//
//   h(M×16)    = obs(M×384) @ Vᵀ(384×16)          GEMM1 on mfma
//   o'(M×384)  = [h|act](M×32) @ [U;D2](32×384)    GEMM2 on mfma
//
// run on v_mfma_f32_16x16x32_bf16 (GEMM2 with K = 32 exactly: 16 h rows
// + 16 action rows; the 17th action is a rank-1 epilogue term).
//
// Blocks: ONE 8-wave block of 16 members per CU (4-wave blocks of 8
// members, two per CU, measured neutral or worse and were dropped).
// All MFMA operands live in LDS: V (GEMM1 B),
// [U;D2] k-major (GEMM2 B) — register fragments for them would push the
// kernel past 256 VGPRs and demote the policy weights to scratch.
//
// Policy phase (act = clamp(W·obsn + b), no shared operand — not
// MFMA-shaped): per-member weights stay in REGISTERS, one 32-lane
// half-wave per member, 12 obs columns per lane (three 8-byte LDS reads),
// 17 accumulators of v_dot2; the first column pair uses the three-operand
// v_dot2 with a constant 0, so no accumulator is zeroed first. Actions
// 0..15 are then reduced with a TRANSPOSING butterfly on the VALU pipe:
// each level a lane keeps half of its accumulators and adds the partner's
// other half (16→8→4→2→1 over lane^1, lane^2, lane^4, lane^8 with DPP
// quad_perm / bank-masked row_shl+row_shr / row_ror, then one v_permlane16_swap add
// across the two rows), so 16 lanes end up with one finished action each —
// 15 DPP adds instead of 16 × 5 full-width ones, in the same summation
// tree. The weight rows are loaded permuted (register a of a lane holds
// action a ^ perm(lane), perm = the lane's low four bits reversed), which
// makes "the half to keep" the low registers on every lane: no level
// selects. Action 16 keeps a plain 5-step DPP reduce into lane 31. The
// tail (bias, clamp, bf16 convert, hact store) then runs ONCE on those 17
// lanes, lane-parallel. The tail lanes also publish the fp32 actions, and
// after the barrier the half-wave reads its member's row back in 16-byte
// words and folds it into Σa² as one fma chain in action order, sliced
// under the GEMM2 epilogue. No ds_bpermute shuffles in the loop (see
// reduce32_dpp).
//
// GEMM1 is wave 0's alone: 24 LDS fragment reads and 12 MFMAs per step,
// ahead of the wave's policy share. It is NOT hidden under the policy
// work: the compiler keeps it as an exec-masked region that wave 0 runs
// through (each MFMA behind its operands' s_waitcnt) before its first
// v_dot2, and the other seven waves wait for wave 0 at the barrier.
// Issuing the MFMAs inside wave 0's dot-product loop (two per 17 v_dot2,
// operands read an iteration ahead, order pinned with sched_group_barrier,
// scalar wave test) was built and measured 70 µs per launch SLOWER
// (T = 1000), so GEMM1 stays a block of its own.
//
// GEMM2 phase: hact is the MFMA A operand, [U;D2] the B operand; a lane's
// D fragment is one obs column of four members. The epilogue treats the
// four rows as the two pairs (0, 1) and (2, 3), in the registers the MFMA
// left them in: the rank-1 term, + c, tanh_fast's multiply, e ± 1 and
// final product, and the fitness fma run two-wide (v_pk_fma_f32,
// v_pk_add_f32, v_pk_mul_f32: each half rounds like the scalar
// instruction), only the clamp, v_exp_f32 and v_rcp_f32 per value; the
// pair is quantized and normalized with one packed bf16 conversion each
// (16-bit LDS stores of its halves). A column's (sum, sumsq) is one pair
// too.
//
// The episode loop exists twice: a block whose 16 slots are all live
// (every block when the population is a multiple of 16) runs a body
// without per-member guards or statistics masks, the last partial block
// the masked body. A live member's instruction sequence is the same in
// both.
//
// rollout_v7_kernel<O, A, true> adds early episode termination for
// `rollout_terminating`: the masked body with an alive bit per member slot
// in place of "slot < live" (protocol at the episode loop). The fixed-length
// instantiation carries none of it.
//
// Every sum keeps the order it had before the transposing reduction, so
// results are bit-identical to the full-width version; and a member's
// arithmetic never depends on its slot (half-wave, wave or block):
// results are bitwise invariant under member_offset sharding.
//
// LDS row strides are padded (OPS = OP+8, KS = 72) — the natural 768 B /
// 128 B strides are ≡ 0 (mod 64 dwords), serializing 16-row fragment
// reads up to 16-way (measured: SQ_LDS_BANK_CONFLICT ≈ 2× SQ_BUSY).
//
// Numerics contract: identical to v6 / rollout_eager (bf16 operands, fp32
// accumulate, quantize-then-normalize obs); tanh via the hardware exp
// unit (~1e-6 rel. error, far below the bf16 quantization of every
// operand).
//
// Layout facts verified on-device (native_probes/mfma_probe.hip):
//   A(16×32): row = lane&15,  k = (lane>>4)*8 + i
//   B(32×16): col = lane&15,  k = (lane>>4)*8 + i
//   D(16×16): col = lane&15,  row = (lane>>4)*4 + reg

#include <hip/hip_runtime.h>

#include <type_traits>

#include "philox.h"
#include "rollout_common.h"

namespace ea {

// out[i] = x[i] + (y[i] of lane^4), i = 0, 1: a partner no single DPP control
// reaches. Banks 0/2 of a row (lanes 0-3, 8-11) read lane+4, banks 1/3
// lane-4, as two bank-masked v_add_f32_dpp into one destination (a lane
// outside the bank mask keeps what it has, so the pair writes every lane
// once). Built from update_dpp this was two zero moves, two masked DPP moves
// and the add per value. The compiler's hazard recognizer cannot see into the
// string: the leading s_nop 1 gives the two wait states a DPP read needs
// after the VALU write of x and y, the trailing one the same for the DPP and
// v_permlane16_swap reads that follow. The outputs are early-clobber, the
// second line of a pair still reads its inputs.
__device__ __forceinline__ void dpp_add_from_xor4_x2(float* out, const float* x, const float* y) {
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %4, %2 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %1, %5, %3 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %4, %2 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %1, %5, %3 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "s_nop 1"
        : "=&v"(out[0]), "=&v"(out[1])
        : "v"(x[0]), "v"(x[1]), "v"(y[0]), "v"(y[1]));
}

// Sum of the two 16-lane rows of a half-wave, in both rows:
// v_permlane16_swap exchanges the odd rows of its first operand with the
// even rows of its second, leaving row 0's x in one result and row 1's in
// the other.
__device__ __forceinline__ float row_pair_add(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    // scalars first: __builtin_bit_cast applied to r[1] directly reads r[0]
    const unsigned from_row0 = r[0], from_row1 = r[1];
    return __builtin_bit_cast(float, from_row0) + __builtin_bit_cast(float, from_row1);
}

typedef __attribute__((ext_vector_type(2))) float floatx2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// Two floats to bf16 with ONE v_cvt_pk_bf16_f32 (a scalar f2b spends the
// same instruction on one value); x is the low half.
__device__ __forceinline__ bf16x2 f2b_pair(floatx2 v) { return __builtin_convertvector(v, bf16x2); }

// ... and back: the low half shifts up, the high half is masked in place.
__device__ __forceinline__ floatx2 b2f_pair(bf16x2 v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const floatx2 f = {__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
    return f;
}

// tanh_fast (rollout_common.h) on two values, the same operations with the
// same roundings: the multiply, e + 1, e - 1 and the final product two-wide,
// the clamp (v_med3_f32), v_exp_f32 and v_rcp_f32 per element, for which no
// two-wide instruction exists. Contraction is off: a caller's add must not
// merge with the final product into an fma.
__device__ __forceinline__ floatx2 tanh_fast_pair(floatx2 x) {
#pragma clang fp contract(off)
    const floatx2 xc = {fminf(fmaxf(x.x, -15.0f), 15.0f), fminf(fmaxf(x.y, -15.0f), 15.0f)};
    const floatx2 t = xc * __builtin_bit_cast(float, 0x4038aa3bu);
    const floatx2 e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    const floatx2 d = e + 1.0f;
    const floatx2 rcp = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    return (e - 1.0f) * rcp;
}

// The first column pair of the policy dot products, acc[a] = w[a][0]·o + 0,
// in the three-operand form v_dot2_f32_bf16 with the inline constant 0: the
// two-operand v_dot2c the builtin selects needs its accumulator zeroed by a
// v_mov first. Several at once (9 + 8: an asm statement takes 30 operands)
// so that one trailing s_nop 2 covers the three wait states a dot result
// needs before another VALU opcode (the v_dot2c of the next pair) may read
// it: the compiler's hazard recognizer cannot see into the string. The
// outputs are early-clobber, a later line still reads its inputs. Whether
// this form rounds like v_dot2c on a zeroed accumulator is not documented;
// on the MI355X it does, in every recorded-bits test
// (tests/golden/rollout_v7_bits*.npz) and in bench.py --dump-outputs.
template <int kCols>
__device__ __forceinline__ void dot2_first_pair9(float* acc, const bf16x2 (*w)[kCols], bf16x2 o2) {
    const unsigned w0 = __builtin_bit_cast(unsigned, w[0][0]);
    const unsigned w1 = __builtin_bit_cast(unsigned, w[1][0]);
    const unsigned w2 = __builtin_bit_cast(unsigned, w[2][0]);
    const unsigned w3 = __builtin_bit_cast(unsigned, w[3][0]);
    const unsigned w4 = __builtin_bit_cast(unsigned, w[4][0]);
    const unsigned w5 = __builtin_bit_cast(unsigned, w[5][0]);
    const unsigned w6 = __builtin_bit_cast(unsigned, w[6][0]);
    const unsigned w7 = __builtin_bit_cast(unsigned, w[7][0]);
    const unsigned w8 = __builtin_bit_cast(unsigned, w[8][0]);
    asm(
        "v_dot2_f32_bf16 %0, %9, %18, 0\n\t"
        "v_dot2_f32_bf16 %1, %10, %18, 0\n\t"
        "v_dot2_f32_bf16 %2, %11, %18, 0\n\t"
        "v_dot2_f32_bf16 %3, %12, %18, 0\n\t"
        "v_dot2_f32_bf16 %4, %13, %18, 0\n\t"
        "v_dot2_f32_bf16 %5, %14, %18, 0\n\t"
        "v_dot2_f32_bf16 %6, %15, %18, 0\n\t"
        "v_dot2_f32_bf16 %7, %16, %18, 0\n\t"
        "v_dot2_f32_bf16 %8, %17, %18, 0\n\t"
        "s_nop 2"
        : "=&v"(acc[0]), "=&v"(acc[1]), "=&v"(acc[2]), "=&v"(acc[3]), "=&v"(acc[4]), "=&v"(acc[5]), "=&v"(acc[6]),
          "=&v"(acc[7]), "=&v"(acc[8])
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(w5), "v"(w6), "v"(w7), "v"(w8),
          "v"(__builtin_bit_cast(unsigned, o2)));
}
template <int kCols>
__device__ __forceinline__ void dot2_first_pair8(float* acc, const bf16x2 (*w)[kCols], bf16x2 o2) {
    const unsigned w0 = __builtin_bit_cast(unsigned, w[0][0]);
    const unsigned w1 = __builtin_bit_cast(unsigned, w[1][0]);
    const unsigned w2 = __builtin_bit_cast(unsigned, w[2][0]);
    const unsigned w3 = __builtin_bit_cast(unsigned, w[3][0]);
    const unsigned w4 = __builtin_bit_cast(unsigned, w[4][0]);
    const unsigned w5 = __builtin_bit_cast(unsigned, w[5][0]);
    const unsigned w6 = __builtin_bit_cast(unsigned, w[6][0]);
    const unsigned w7 = __builtin_bit_cast(unsigned, w[7][0]);
    asm(
        "v_dot2_f32_bf16 %0, %8, %16, 0\n\t"
        "v_dot2_f32_bf16 %1, %9, %16, 0\n\t"
        "v_dot2_f32_bf16 %2, %10, %16, 0\n\t"
        "v_dot2_f32_bf16 %3, %11, %16, 0\n\t"
        "v_dot2_f32_bf16 %4, %12, %16, 0\n\t"
        "v_dot2_f32_bf16 %5, %13, %16, 0\n\t"
        "v_dot2_f32_bf16 %6, %14, %16, 0\n\t"
        "v_dot2_f32_bf16 %7, %15, %16, 0\n\t"
        "s_nop 2"
        : "=&v"(acc[0]), "=&v"(acc[1]), "=&v"(acc[2]), "=&v"(acc[3]), "=&v"(acc[4]), "=&v"(acc[5]), "=&v"(acc[6]),
          "=&v"(acc[7])
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(w5), "v"(w6), "v"(w7),
          "v"(__builtin_bit_cast(unsigned, o2)));
}

// Compile-time geometry and the dynamic-LDS layout (byte offsets), stated
// once for the kernel's carve-up and the launcher's footprint.
template <int O, int A>
struct V7Layout {
    static constexpr int kWaves = 8;
    static constexpr int kM = 2 * kWaves;           // members per block
    static constexpr int OP = (O + 127) / 128 * 128;
    static constexpr int OPS = OP + 8;              // padded obs-row stride (bank decorrelation)
    static constexpr int KS = 72;                   // padded hact row stride (vs 64)
    static constexpr int KU = 40;                   // ud row stride: 32 + 8 pad (bank decorrelation)
    static constexpr int AF = (A + 1 + 3) / 4 * 4;  // actf row stride (16-byte rows)

    static constexpr int obs = 0;                           // bf16 [kM][OPS] raw (quantized) obs
    static constexpr int obsn = obs + kM * OPS * 2;         // bf16 [kM][OPS] normalized obs
    static constexpr int hact = obsn + kM * OPS * 2;        // bf16 [16][KS]: k<16 h, k=16..31 act[0..16), slot 32 = act[16]
    static constexpr int v = hact + 16 * KS * 2;            // bf16 [16][OPS] V (GEMM1 B-operand)
    static constexpr int actf = v + 16 * OPS * 2;           // float [kM][AF] fp32 actions of the step; slot A: Σa² at wrap-up
    static constexpr int c = actf + kM * AF * 4;            // float [OP]
    static constexpr int wr = c + OP * 4;                   // float [OP]
    static constexpr int mean = wr + OP * 4;                // float [OP]
    static constexpr int istd = mean + OP * 4;              // float [OP]
    static constexpr int wave_fit = istd + OP * 4;          // float [kWaves][16] fitness partials
    static constexpr int d2last = wave_fit + kWaves * 16 * 4;  // float [OP] D2_T row A-1 (rank-1 epilogue term)
    static constexpr int ud = d2last + OP * 4;              // bf16 [OP][KU] k-major GEMM2 B
    static constexpr int alive = ud + OP * KU * 2;          // unsigned: bit m = member slot m still runs (kTerm only)
    static constexpr int bytes = alive + 16;
    static_assert(bytes <= 160 * 1024, "v7 LDS footprint exceeds the 160 KB of a gfx950 workgroup");
    static_assert(actf % 16 == 0 && ud % 16 == 0 && v % 16 == 0 && alive % 4 == 0, "misaligned LDS region");
    // the policy phase reads a lane's obsn chunk as 8-byte words
    static_assert(obsn % 8 == 0 && (OPS * 2) % 8 == 0 && (OP / 32) % 4 == 0, "misaligned policy obs chunk");
};

// All guards constant-fold: a runtime-guarded W-load was measured to
// demote w_frag to scratch memory.
// kTerm adds early episode termination (see the alive-mask protocol at the
// episode loop); everything it needs sits behind `if constexpr (kTerm)`, and
// a live member runs the same arithmetic sequence in both instantiations.
template <int O, int A, bool kTerm>
__global__ __launch_bounds__((64 * V7Layout<O, A>::kWaves), 1) void rollout_v7_kernel(RolloutArgs args) {
    using L = V7Layout<O, A>;
    constexpr int kWaves = L::kWaves, kM = L::kM, OP = L::OP, OPS = L::OPS, KS = L::KS, KU = L::KU, AF = L::AF;
    constexpr int kThreads = 64 * kWaves;
    constexpr int A_MAX = A;
    constexpr int R = 16;
    constexpr int kTiles = OP / 16;           // GEMM2 output tiles
    constexpr int kTilesPerWave = kTiles / kWaves;
    constexpr int kChunk = OP / 32;           // policy obs columns per lane (12)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int base_member = blockIdx.x * kM;
    if (base_member >= args.n_members) return;
    const int live = min(kM, args.n_members - base_member);

    extern __shared__ unsigned char lds7[];
    __bf16* obs_l = reinterpret_cast<__bf16*>(lds7 + L::obs);
    __bf16* obsn_l = reinterpret_cast<__bf16*>(lds7 + L::obsn);
    __bf16* hact_l = reinterpret_cast<__bf16*>(lds7 + L::hact);
    __bf16* v_l = reinterpret_cast<__bf16*>(lds7 + L::v);
    float* actf_l = reinterpret_cast<float*>(lds7 + L::actf);
    float* c_l = reinterpret_cast<float*>(lds7 + L::c);
    float* wr_l = reinterpret_cast<float*>(lds7 + L::wr);
    float* mean_l = reinterpret_cast<float*>(lds7 + L::mean);
    float* istd_l = reinterpret_cast<float*>(lds7 + L::istd);
    float* wave_fit = reinterpret_cast<float*>(lds7 + L::wave_fit);
    float* d2last_l = reinterpret_cast<float*>(lds7 + L::d2last);
    __bf16* ud_l = reinterpret_cast<__bf16*>(lds7 + L::ud);
    [[maybe_unused]] unsigned* alive_l = reinterpret_cast<unsigned*>(lds7 + L::alive);

    const EnvBlob env(args.env_blob, O, A, R);
    const long AO = (long)A * O;

    // ---- stage vectors (pads: c=0, wr=0, mean=0, istd=0 → obsn pad = 0) ----
    for (int j = tid; j < OP; j += kThreads) {
        const bool in = j < O;
        c_l[j] = in ? env.c[j] : 0.0f;
        wr_l[j] = in ? env.wr[j] : 0.0f;
        mean_l[j] = in ? env.mean[j] : 0.0f;
        istd_l[j] = in ? 1.0f / env.std[j] : 0.0f;
        // act[A-1]'s D2 row is applied as a rank-1 epilogue term (bf16-
        // quantized like the mfma operands) so the GEMM K stays 32
        d2last_l[j] = in ? b2f(f2b(env.D2_T[(long)(A - 1) * O + j])) : 0.0f;
    }
    for (int j = tid; j < 16 * KS; j += kThreads) hact_l[j] = f2b(0.0f);
    for (int j = tid; j < kM * AF; j += kThreads) actf_l[j] = 0.0f;
    // alive mask: the bits of the live slots; an empty slot's bit is never set
    if constexpr (kTerm) {
        if (tid == 0) *alive_l = (1u << live) - 1u;
    }

    // GEMM1 B (V) in LDS (only wave 0 reads it — registers on every wave
    // would blow the VGPR budget and demote w_frag to scratch).
    for (int j = tid; j < 16 * OPS; j += kThreads) {
        const int r = j / OPS, o = j % OPS;
        v_l[j] = (r < R && o < O) ? f2b(env.V[(long)r * O + o]) : f2b(0.0f);
    }

    const int g2_row = lane & 15;              // A-frag row (member) for GEMM2/GEMM1
    const int g2_k0 = (lane >> 4) * 8;
    const int c_col = lane & 15;               // C-frag col
    const int c_row0 = (lane >> 4) * 4;        // C-frag first row (member)

    // GEMM2 B ([U;D2 rows 0..15]): K = 32 exactly (R=16 h-rows + 16 action
    // rows; action A-1 is the rank-1 epilogue term), k-major LDS with
    // padded stride KU.
    for (int j = tid; j < OP * KU; j += kThreads) {
        const int o = j / KU, k = j % KU;
        float v = 0.0f;
        if (o < O && k < 32) {
            if (k < R) v = env.U_T[(long)k * O + o];
            else if (k - R < A - 1) v = env.D2_T[(long)(k - R) * O + o];
        }
        ud_l[j] = f2b(v);
    }

    // ---- per-member policy weights in registers -----------------------------
    // half-wave (32 lanes) per member: member = 2*wave + (lane>>5);
    // lane owns obsn columns [l32*kChunk, l32*kChunk + kChunk).
    // Register a < 16 holds weight row a ^ perm, perm being the lane's low
    // four bits reversed: the transposing reduction of the policy phase then
    // needs no per-lane choice of what to keep (see there). Row 16 stays put.
    static_assert(A_MAX == 17, "the policy reduction is laid out for 16 butterfly actions and one plain one");
    const int l32 = lane & 31;
    const int my_member = 2 * wave + (lane >> 5);
    const int perm = ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
    bf16x2 w_frag[A_MAX][kChunk / 2];
    {
        const float* W = args.params + (long)(base_member + min(my_member, live - 1)) * ((long)A * O + A);
        const int cbase = l32 * kChunk;
#pragma unroll
        for (int a = 0; a < A_MAX; ++a) {
            const float* Wa = W + (long)(a < 16 ? (a ^ perm) : a) * O;
#pragma unroll
            for (int p = 0; p < kChunk / 2; ++p) {
                const int k0 = cbase + 2 * p;
                bf16x2 w2;
                w2.x = (k0 < O) ? f2b(Wa[k0]) : f2b(0.0f);
                w2.y = (k0 + 1 < O) ? f2b(Wa[k0 + 1]) : f2b(0.0f);
                w_frag[a][p] = w2;
            }
        }
    }

    // After the transposing reduction (see the policy phase) the first 16
    // lanes of the half-wave hold one finished action each; its lane 31
    // holds action A-1 from the plain reduction. Those 17 lanes run the tail.
    const int my_act = (l32 == 31) ? 16 : perm;
    const bool tail_lane = my_member < live && my_act < A && (l32 < 16 || l32 == 31);
    const float my_bias =
        tail_lane ? args.params[(long)(base_member + my_member) * (AO + A) + AO + my_act] : 0.0f;
    __bf16* my_hact = hact_l + my_member * KS + ((my_act < 16) ? (16 + my_act) : 32);
    float* my_actf = actf_l + my_member * AF + my_act;
    // kTerm: the lane's epilogue column of tile tw is health_index when this
    // equals 16 * tw (one compare per tile; at most four lanes of one wave,
    // one per 16-lane row group, ever match)
    [[maybe_unused]] const int health_rel = args.health_index - (wave * kTilesPerWave * 16 + c_col);

    // ---- initial observations (philox stream per global member) -------------
    for (int j = tid; j < kM * OPS; j += kThreads) obs_l[j] = f2b(0.0f);
    __syncthreads();
    {
        const int per_member4 = (O + 3) / 4;
        for (int idx = tid; idx < kM * per_member4; idx += kThreads) {
            const int m = idx / per_member4;
            const int j4 = idx % per_member4;
            if (m >= live) continue;
            float z[4];
            const unsigned long long iseed = args.seed_ptr ? *args.seed_ptr : args.init_seed;
            philox_normal4(iseed, (uint32_t)(args.member_offset + base_member + m), (uint64_t)j4, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j4 * 4 + u;
                if (j < O) obs_l[m * OPS + j] = f2b(0.1f * z[u]);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < kM * OPS; j += kThreads) {
        const int jo = j % OPS;
        obsn_l[j] = (jo < OP) ? f2b((b2f(obs_l[j]) - mean_l[jo]) * istd_l[jo]) : f2b(0.0f);
    }
    __syncthreads();

    // Per-column constants of the lane's GEMM2 epilogue columns. They do not
    // change during the episode, and a load inside the step loop cannot be
    // hoisted over its barriers by the compiler, so read them once, here
    // (staged before the barriers above).
    float d2last_r[kTilesPerWave], c_r[kTilesPerWave], wr_r[kTilesPerWave], mean_r[kTilesPerWave],
        istd_r[kTilesPerWave];
#pragma unroll
    for (int tw = 0; tw < kTilesPerWave; ++tw) {
        const int col = (wave * kTilesPerWave + tw) * 16 + c_col;
        d2last_r[tw] = d2last_l[col];
        c_r[tw] = c_l[col];
        wr_r[tw] = wr_l[col];
        mean_r[tw] = mean_l[col];
        istd_r[tw] = istd_l[col];
    }

    // ---- episode state in registers ----
    floatx2 fit_part[2] = {};                  // member rows (lane>>4)*4 + {0,1}, {2,3} of GEMM2
    float actsq_total = 0.0f;                  // my_member's Σa² (lane 31 of the half-wave publishes it)
    floatx2 stat[kTilesPerWave] = {};          // (sum, sumsq) per owned obs column
    [[maybe_unused]] int len = 0;              // kTerm: my_member's episode length (lane 31 publishes it)

    // the 16 rows of an MFMA A/D fragment are exactly the block's member slots
    static_assert(kM == 16, "GEMM1/GEMM2 fragments address member rows 0..15 unguarded");
    const int a_row = g2_row;

    // The episode loop, instantiated twice: kFull for a block whose kM
    // member slots are all live (every block of a population that is a
    // multiple of kM), without the per-member guards; and the masked body
    // for the last, partial block. A live member runs the same instruction
    // sequence in both, so its results do not depend on which one it is in.
    //
    // Termination (kTerm) runs the masked body alone, with "slot < live"
    // replaced by the slot's bit of the alive mask (the bits of slots >= live
    // are never set, so the one mask serves both purposes). The mask is one
    // LDS word. Every thread reads it at the top of a step and moves it to a
    // scalar register, so the member tests of the step test a scalar and the
    // exit is block-uniform. The bits are cleared in the GEMM2 epilogue by the
    // lanes that own column health_index, with an integer atomicAnd (order-
    // independent, deterministic). The read comes after the end-of-step
    // barrier (the staging barriers for step 0) and before the mid-step
    // barrier; the next clear comes after the mid-step barrier and before the
    // end-of-step one: no race and no extra barrier. From the step after its
    // death a member's fit_part, statistics, Σa² and length stay as they are
    // (selects and skipped adds, never a zero multiplier: a dead row's later
    // observations are whatever the closed loop makes of them). Its rows of
    // obs, obsn and hact keep being computed, which no live member sees: row
    // m of an MFMA result depends on row m of A alone, and the policy phase
    // reads a member's own obsn row only.
    auto episode = [&](auto full) __attribute__((always_inline)) {
    constexpr bool kFull = decltype(full)::value;
    static_assert(!(kTerm && kFull), "the terminating kernel runs the masked body");
    for (int t = 0; t < args.steps; ++t) {
        [[maybe_unused]] unsigned alive = 0;       // scalar: this step's alive mask
        [[maybe_unused]] unsigned rows_alive = 0;  // bit r: GEMM2 row c_row0 + r runs
        [[maybe_unused]] bool member_on = true;    // my_member runs
        if constexpr (kTerm) {
            alive = __builtin_amdgcn_readfirstlane(*alive_l);
            if (alive == 0) break;
            rows_alive = alive >> c_row0;
            member_on = (alive >> my_member) & 1u;
            len += member_on;
        }
        // ===== GEMM1 (wave 0): h = obs @ Vᵀ, before the wave's policy share
        // (not overlapped with it, see the header) =====
        floatx4 h_acc = {0.f, 0.f, 0.f, 0.f};
        if (wave == 0) {
            // two accumulator chains: a single accumulator serializes 12
            // dependent MFMAs (~32 cycles each) on wave 0, which is the
            // barrier straggler (it also runs its policy share)
            floatx4 h_acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < OP / 32; s += 2) {
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(obs_l + a_row * OPS + s * 32 + g2_k0);
                const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(v_l + c_col * OPS + s * 32 + g2_k0);
                h_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, h_acc, 0, 0, 0);
                const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(obs_l + a_row * OPS + (s + 1) * 32 + g2_k0);
                const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(v_l + c_col * OPS + (s + 1) * 32 + g2_k0);
                h_acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, h_acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) h_acc[r] += h_acc1[r];
        }
        // ===== policy: act = clamp(W · obsn + b) — per-member half-waves =====
        {
            float acc[A_MAX];
#pragma unroll
            for (int a = 0; a < A_MAX; ++a) acc[a] = 0.0f;  // for the masked body's dead members only
            if (kFull || (kTerm ? member_on : my_member < live)) {
                // the lane's chunk as 8-byte reads (ds_read_b64), two column pairs each
                const bf16x4* on = reinterpret_cast<const bf16x4*>(obsn_l + my_member * OPS + l32 * kChunk);
#pragma unroll
                for (int p = 0; p < kChunk / 2; ++p) {
                    const bf16x4 o4 = on[p / 2];
                    const bf16x2 o2 = (p & 1) ? __builtin_shufflevector(o4, o4, 2, 3)
                                              : __builtin_shufflevector(o4, o4, 0, 1);
                    if (p == 0) {
                        dot2_first_pair9(acc, w_frag, o2);
                        dot2_first_pair8(acc + 9, w_frag + 9, o2);
                        continue;
                    }
#pragma unroll
                    for (int a = 0; a < A_MAX; ++a) {
                        acc[a] = __builtin_amdgcn_fdot2_f32_bf16(w_frag[a][p], o2, acc[a], false);
                    }
                }
            }
            // Transposing reduction of actions 0..15 over the half-wave's
            // 32 lanes: every level halves the accumulators a lane still
            // carries (16→8→4→2→1) while it doubles the lanes summed into
            // them, 15 DPP adds instead of 16 × 5 full-width ones. The
            // levels pair lane^1, lane^2, lane^4, lane^8 and finally the
            // two rows — the same balanced tree, pair for pair, as the
            // row_shr 1/2/4/8 + row_bcast reduction action 16 still uses,
            // so every action sum has one summation order (and the bits
            // the full-width reduction gave).
            // No level selects what to keep: register i holds action
            // i ^ perm, and the lane^1 partner (perm' = perm ^ 8) holds
            // that same action in its register i + 8, since
            // (i + 8) ^ perm' = i ^ perm for i < 8; likewise lane^2 with
            // i + 4, lane^4 with i + 2 and lane^8 with i + 1. So a lane
            // always keeps its low half and adds the partner's high half,
            // and ends with action 0 ^ perm = my_act in register 0.
            // Identical in both half-waves and every wave, so a member's
            // arithmetic does not depend on its slot.
            float v8[8], v4[4], v2[2];
#pragma unroll
            for (int i = 0; i < 8; ++i) v8[i] = dpp_add_from<0xB1>(acc[i], acc[i + 8]);  // quad_perm:[1,0,3,2]
#pragma unroll
            for (int i = 0; i < 4; ++i) v4[i] = dpp_add_from<0x4E>(v8[i], v8[i + 4]);    // quad_perm:[2,3,0,1]
            dpp_add_from_xor4_x2(v2, v4, v4 + 2);
            const float a_sum = row_pair_add(dpp_add_from<0x128>(v2[0], v2[1]));         // row_ror:8
            const float a_last = reduce32_dpp(acc[A_MAX - 1]);
            if (tail_lane) {
                const float av = fminf(fmaxf(((l32 == 31) ? a_last : a_sum) + my_bias, -1.0f), 1.0f);
                *my_hact = f2b(av);
                *my_actf = av;
            }
        }
        // h goes to hact only here, after wave 0's policy share. Storing it
        // at the end of the GEMM1 region takes four v_mov 0 off every wave
        // but measured 17 µs per launch slower (T = 1000): wave 0 is the
        // barrier straggler, and the conversions and stores then sit ahead
        // of its dot products.
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // D: col = h-index, row = member
                const int m = c_row0 + r;
                hact_l[m * KS + c_col] = f2b(h_acc[r]);
            }
        }
        __syncthreads();

        // ===== GEMM2: o' = tanh(hact @ [U;D2] + act16·d2last + c) =====
        {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(hact_l + g2_row * KS + g2_k0);
            // per-member act[A-1] for the rank-1 term, indexed by C rows
            floatx2 a16[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int m = c_row0 + 2 * q;
                a16[q].x = b2f(hact_l[m * KS + 32]);
                a16[q].y = b2f(hact_l[(m + 1) * KS + 32]);
            }
            // Σa² of the step, as ONE fma chain in action order per member
            // (the summation order the fitness has always had), from the
            // fp32 actions the tail lanes just published. Every lane of the
            // half-wave runs its member's chain, branch-free and a slice
            // per tile, so its LDS and fma latencies hide under the
            // epilogue; only lane 31's copy is used at wrap-up. The row is
            // read as 16-byte words (ds_read_b128), each in the tile that
            // first needs it.
            constexpr int kSqPerTile = (A_MAX + kTilesPerWave - 1) / kTilesPerWave;
            const floatx4* af = reinterpret_cast<const floatx4*>(actf_l + my_member * AF);
            floatx4 av[AF / 4];
            float sq = 0.0f;
#pragma unroll
            for (int tw = 0; tw < kTilesPerWave; ++tw) {
#pragma unroll
                for (int w = 0; w < AF / 4; ++w) {
                    // the tile whose slice [a_lo, a_hi) holds the word's first action
                    const int a_lo = tw * kSqPerTile, a_hi = min(a_lo + kSqPerTile, A_MAX);
                    if (4 * w >= a_lo && 4 * w < a_hi) av[w] = af[w];
                }
                const int col = (wave * kTilesPerWave + tw) * 16 + c_col;
                floatx4 acc = {0.f, 0.f, 0.f, 0.f};
                const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(ud_l + col * KU + g2_k0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
                const floatx2 d2l = {d2last_r[tw], d2last_r[tw]};
                const floatx2 cv = {c_r[tw], c_r[tw]};
                const floatx2 wrv = {wr_r[tw], wr_r[tw]};
                const floatx2 mv = {mean_r[tw], mean_r[tw]};
                const floatx2 iv = {istd_r[tw], istd_r[tw]};
                // The four rows as the two pairs (0, 1) and (2, 3), which the
                // MFMA result already holds in consecutive registers: every
                // step of the epilogue that has a two-wide fp32 instruction
                // (v_pk_fma_f32, v_pk_add_f32, v_pk_mul_f32; each half rounds
                // like the scalar instruction) runs once per pair.
                floatx2 o_pair[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const floatx2 accq = {acc[2 * q], acc[2 * q + 1]};
                    o_pair[q] = tanh_fast_pair(__builtin_elementwise_fma(a16[q], d2l, accq) + cv);
                    const floatx2 fit_next = __builtin_elementwise_fma(wrv, o_pair[q], fit_part[q]);
                    if constexpr (kTerm) {
                        // a dead row keeps the sum it died with
                        fit_part[q].x = ((rows_alive >> (2 * q)) & 1u) ? fit_next.x : fit_part[q].x;
                        fit_part[q].y = ((rows_alive >> (2 * q + 1)) & 1u) ? fit_next.y : fit_part[q].y;
                    } else {
                        fit_part[q] = fit_next;
                    }
                }
                // Statistics over the live rows, one chain in row order per
                // column. Pad columns (col >= O) need no mask: their c, d2last
                // and [U;D2] row are 0, so o = tanh_fast(0) = +0 exactly, and
                // their sums are never stored. Row 0 starts the sums: 0 + o
                // and fma(o, o, 0) give the same bits (tanh_fast never
                // returns -0) but cost an op each.
                const float o_row[4] = {o_pair[0].x, o_pair[0].y, o_pair[1].x, o_pair[1].y};
                float ssum = 0.0f, ssq = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = kFull || (kTerm ? ((rows_alive >> r) & 1u) != 0 : c_row0 + r < live);
                    if (r == 0) {
                        ssum = in ? o_row[r] : 0.0f;
                        ssq = in ? o_row[r] * o_row[r] : 0.0f;
                    } else if (in) {
                        // o is a product ((e - 1) · rcp): without this the
                        // unmasked body contracts it into the add as one fma
                        // (one rounding instead of two), and the sums change bits
#pragma clang fp contract(off)
                        ssum += o_row[r];
                        ssq = fmaf(o_row[r], o_row[r], ssq);
                    }
                }
                // quantize, normalize and store the rows in pairs: one packed
                // conversion serves two rows (same values as row by row)
                [[maybe_unused]] floatx2 health[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const bf16x2 ob = f2b_pair(o_pair[q]);
                    const floatx2 of = b2f_pair(ob);
                    const bf16x2 on = f2b_pair((of - mv) * iv);
                    __bf16* po = obs_l + (c_row0 + 2 * q) * OPS + col;
                    __bf16* pn = obsn_l + (c_row0 + 2 * q) * OPS + col;
                    po[0] = ob.x;
                    po[OPS] = ob.y;
                    pn[0] = on.x;
                    pn[OPS] = on.y;
                    if constexpr (kTerm) health[q] = of;
                }
                if constexpr (kTerm) {
                    // Done after this step: the bf16 value the policy would
                    // see next is outside the healthy range (a NaN is
                    // outside). Only the lanes whose column is health_index
                    // get here, the other waves branch over it.
                    if (health_rel == 16 * tw) {
                        const float h4[4] = {health[0].x, health[0].y, health[1].x, health[1].y};
                        unsigned dead = 0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (!(args.healthy_lo <= h4[r] && h4[r] <= args.healthy_hi)) dead |= 1u << r;
                        }
                        if (dead != 0) atomicAnd(alive_l, ~(dead << c_row0));
                    }
                }
                // the column's running sum and sum of squares as one pair:
                // one packed add, and nothing to pair across tiles
                {
                    const floatx2 tile_stat = {ssum, ssq};
                    stat[tw] += tile_stat;
                }
#pragma unroll
                for (int u = 0; u < kSqPerTile; ++u) {
                    const int a = tw * kSqPerTile + u;
                    if (a < A_MAX) sq = fmaf(av[a / 4][a % 4], av[a / 4][a % 4], sq);
                }
            }
            if constexpr (kTerm) {
                // a dead member's row still holds its last actions
                if (member_on) actsq_total += sq;
            } else {
                actsq_total += sq;
            }
        }
        __syncthreads();
    }
    };
    if constexpr (kTerm) {
        episode(std::false_type{});
    } else {
        if (live == kM) episode(std::true_type{});
        else episode(std::false_type{});
    }

    // ---- wrap-up ----
    // Deterministic fitness reduction (no float atomics — the kernel must
    // be bitwise run-to-run reproducible): (1) shuffle-reduce fit_part
    // across the 16 lanes of each row segment, (2) stage per-wave partials
    // in LDS, (3) one thread per member sums the waves in fixed order.
    float fit_row[4] = {fit_part[0].x, fit_part[0].y, fit_part[1].x, fit_part[1].y};
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) fit_row[r] += __shfl_down(fit_row[r], off, 16);
    }
    if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) wave_fit[wave * 16 + c_row0 + r] = fit_row[r];
    }
    if (l32 == 31 && my_member < live) {
        actf_l[my_member * AF + A_MAX] = actsq_total;
        if constexpr (kTerm) {
            // the length rides beside Σa² (its bits in a float slot)
            static_assert(AF >= A_MAX + 2, "no free actf slot for the episode length");
            actf_l[my_member * AF + A_MAX + 1] = __builtin_bit_cast(float, len);
        }
    }
    __syncthreads();
    if (tid < live) {
        float total = 0.0f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += wave_fit[w * 16 + tid];
        // the alive bonus is paid per step survived
        int steps_m = args.steps;
        if constexpr (kTerm) steps_m = __builtin_bit_cast(int, actf_l[tid * AF + A_MAX + 1]);
        args.fitness_out[base_member + tid] =
            total + args.alive_bonus * (float)steps_m - args.act_cost * actf_l[tid * AF + A_MAX] / (float)A;
        if constexpr (kTerm) args.steps_out[base_member + tid] = steps_m;
    }
    // per-block stat slice: the four 16-lane groups of a wave share each
    // col (they hold different member rows), so reduce across them with
    // fixed-order shuffles, then lanes 0-15 store — plain stores, no
    // float atomics, run-to-run deterministic
    float* stats = args.obs_stats_out + (int64_t)blockIdx.x * 2 * O;
#pragma unroll
    for (int tw = 0; tw < kTilesPerWave; ++tw) {
        float ss = stat[tw].x, sq = stat[tw].y;
        ss += __shfl_down(ss, 32, 64);
        ss += __shfl_down(ss, 16, 64);
        sq += __shfl_down(sq, 32, 64);
        sq += __shfl_down(sq, 16, 64);
        const int col = (wave * kTilesPerWave + tw) * 16 + c_col;
        if (lane < 16 && col < O) {
            stats[col] = ss;
            stats[O + col] = sq;
        }
    }
}

template <int O_T, int A_T, bool kTerm>
static void launch_v7(const RolloutArgs& args, int n, hipStream_t stream) {
    using L = V7Layout<O_T, A_T>;
    static_assert(L::kM == kV7MembersPerBlock, "the dispatcher sizes the stat partials by kV7MembersPerBlock");
    static bool attr_set = false;
    if (!attr_set) {
        allow_max_dynamic_lds(reinterpret_cast<const void*>(&rollout_v7_kernel<O_T, A_T, kTerm>));
        attr_set = true;
    }
    const int blocks = (n + L::kM - 1) / L::kM;
    hipLaunchKernelGGL((rollout_v7_kernel<O_T, A_T, kTerm>), dim3(blocks), dim3(64 * L::kWaves), L::bytes, stream,
                       args);
}

void launch_rollout_v7(const RolloutArgs& args, int n, hipStream_t stream, bool terminating) {
    constexpr int O_T = 376, A_T = 17;
    TORCH_CHECK(args.obs_dim == O_T && args.act_dim == A_T && args.rank == 16 && args.hidden == 0,
                "rollout v7 is instantiated for the linear policy at the Humanoid geometry (obs 376, act 17, rank 16)");
    if (terminating) {
        TORCH_CHECK(args.steps_out != nullptr && args.health_index >= 0 && args.health_index < O_T,
                    "terminating rollout v7 needs steps_out and a health_index in [0, ", O_T, ")");
        launch_v7<O_T, A_T, true>(args, n, stream);
    } else {
        launch_v7<O_T, A_T, false>(args, n, stream);
    }
}

}  // namespace ea
