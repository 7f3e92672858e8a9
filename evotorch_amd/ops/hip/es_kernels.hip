// K1 / K3 / K4 kernels: Gaussian population sampling,
// fused ES gradient reductions, fused optimizer steps — gfx950 (CDNA4).
//
// Design notes (MI355X):
// * Sampling is HBM-write-bound: each thread produces 4 normals from one
//   philox counter and stores them contiguously (16 B/lane stores, the
//   coalescing sweet spot). The antithetic mirror writes the second half
//   of the population in the same pass — one kernel, one read of mu/sigma
//   (which L2-caches), ~N*L*4 bytes written.
// * Gradients are HBM-read-bound (read X once): grid = column tiles ×
//   row chunks; each block reduces its row chunk for 256 consecutive
//   columns (fully coalesced across the wave) and atomically adds its
//   fp32 partials — the fused kernel produces BOTH mu_grad and sigma_grad
//   from the single pass over X, halving traffic vs two library GEMVs.
// * ClipUp is three tiny kernels chained on the stream (norm, update+norm,
//   scale) — no host synchronization anywhere. PGPE's whole update (ClipUp,
//   mu + velocity, bounded sigma step) also exists as ONE single-block
//   kernel with the same bits (gaussian_clipup_update).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "check.h"
#include "philox.h"
#include "reduce.h"

namespace ea {

// Run `...` with T bound to the tensor's element type (fp64, fp32, fp16, bf16).
#define DISPATCH_FLOAT_T(tensor, name, ...)                                                                    \
    AT_DISPATCH_FLOATING_TYPES_AND2(at::ScalarType::BFloat16, at::ScalarType::Half, (tensor).scalar_type(), name, \
                                    [&] { using T = scalar_t; __VA_ARGS__ })

// ---------------------------------------------------------------------------
// K1: sampling
// ---------------------------------------------------------------------------

// Graph-safe seeding: when `seed_ptr` is non-null the philox seed is read
// from device memory (and a separate bump kernel advances it), so a
// hipGraph replay of the sampling kernel produces a fresh population each
// replay — a by-value seed would be frozen into the captured graph.
__device__ __forceinline__ uint64_t resolve_seed(uint64_t seed, const unsigned long long* seed_ptr) {
    return seed_ptr ? (uint64_t)*seed_ptr : seed;
}

__global__ void bump_seed_kernel(unsigned long long* seed_ptr) {
    // splitmix64 advance (single thread)
    unsigned long long x = *seed_ptr + 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    *seed_ptr = (z ^ (z >> 31)) & 0x7FFFFFFFFFFFFFFFull;
}

// Counter addressing is STREAM-PER-ROW: row r of the (virtual, possibly
// rank-sharded) population draws from philox stream `row_offset + r` with
// the counter walking the row's columns (counter c covers columns
// [4c, 4c+4)). Any row partition of the population is therefore
// regenerable exactly, for ANY solution length — the property the SPMD
// sharded sampling and the streaming large-L gradient path both rely on
// (SURVEY.md §7 "RNG discipline"). CPU reference:
// evotorch_amd/neuroevolution/philox_ref.py::philox_normals_2d.
template <typename T, bool kSymmetric>
__global__ void sample_gaussian_kernel(T* __restrict__ out, const T* __restrict__ mu, const T* __restrict__ sigma,
                                       int64_t rows,  // = N (plain) or N/2 (symmetric)
                                       int64_t length, uint64_t seed_in,
                                       const unsigned long long* __restrict__ seed_ptr,
                                       int64_t row_offset) {
    const uint64_t seed = resolve_seed(seed_in, seed_ptr);
    const int64_t len4 = (length + 3) / 4;
    const int64_t total4 = rows * len4;
    for (int64_t idx4 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx4 < total4;
         idx4 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx4 / len4;
        const int64_t col4 = idx4 - row * len4;
        float z[4];
        philox_normal4(seed, (uint32_t)(row + row_offset), (uint64_t)col4, z);
        const int64_t base_col = col4 * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t col = base_col + j;
            if (col >= length) break;
            const float m = static_cast<float>(mu[col]);
            const float s = static_cast<float>(sigma[col]);
            const float plus = fmaf(s, z[j], m);
            out[row * length + col] = static_cast<T>(plus);
            if (kSymmetric) {
                out[(row + rows) * length + col] = static_cast<T>(2.0f * m - plus);
            }
        }
    }
}

// fp32 fast path for length % 4 == 0: the 4 philox normals of one counter
// are 4 consecutive elements of one row, stored as a single 16 B float4
// (the CDNA coalescing sweet spot — cdna_hip_programming.md G13); mu and
// sigma are read as float4 too.
template <bool kSymmetric>
__global__ void sample_gaussian_f32x4_kernel(float4* __restrict__ out, const float4* __restrict__ mu,
                                             const float4* __restrict__ sigma, int64_t rows, int64_t length4,
                                             uint64_t seed_in, const unsigned long long* __restrict__ seed_ptr,
                                             int64_t row_offset) {
    const uint64_t seed = resolve_seed(seed_in, seed_ptr);
    const int64_t total4 = rows * length4;
    for (int64_t idx4 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx4 < total4;
         idx4 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx4 / length4;
        const int64_t col4 = idx4 - row * length4;
        float z[4];
        philox_normal4(seed, (uint32_t)(row + row_offset), (uint64_t)col4, z);
        const float4 m = mu[col4];
        const float4 s = sigma[col4];
        float4 plus;
        plus.x = fmaf(s.x, z[0], m.x);
        plus.y = fmaf(s.y, z[1], m.y);
        plus.z = fmaf(s.z, z[2], m.z);
        plus.w = fmaf(s.w, z[3], m.w);
        out[idx4] = plus;
        if (kSymmetric) {
            float4 minus;
            minus.x = 2.0f * m.x - plus.x;
            minus.y = 2.0f * m.y - plus.y;
            minus.z = 2.0f * m.z - plus.z;
            minus.w = 2.0f * m.w - plus.w;
            out[idx4 + total4] = minus;
        }
    }
}

// Operands of the sampling-shaped entry points: `out` is N x L, mu and sigma
// are dense L-vectors of its dtype. Returns the rows a launch generates
// (N, or N/2 mirrored directions when symmetric).
static int64_t check_sampling_operands(const torch::Tensor& out, const torch::Tensor& mu, const torch::Tensor& sigma,
                                       bool symmetric) {
    check_primary(out, "out", 2);
    check_operand(mu, "mu", out, out.size(1));
    check_operand(sigma, "sigma", out, out.size(1));
    TORCH_CHECK(!symmetric || out.size(0) % 2 == 0, "symmetric sampling needs even popsize, got ", out.size(0));
    return symmetric ? out.size(0) / 2 : out.size(0);
}

static void sample_gaussian_impl(torch::Tensor out, torch::Tensor mu, torch::Tensor sigma, bool symmetric, int64_t seed,
                                 const unsigned long long* seed_ptr, int64_t row_offset = 0) {
    TORCH_CHECK(row_offset >= 0, "row_offset must be non-negative");
    const int64_t rows = check_sampling_operands(out, mu, sigma, symmetric);
    const int64_t length = out.size(1);
    const int threads = 256;
    // 2048 blocks (8/CU) saturate: deeper grids measured identical (the
    // SQ_WAIT:BUSY ~12:1 is philox->Box-Muller dependency latency plus the
    // write pipe, not occupancy starvation)
    const int blocks = grid_for(rows * ((length + 3) / 4), threads, 256 * 8);
    auto stream = at::cuda::getCurrentCUDAStream();
    if (out.scalar_type() == at::ScalarType::Float && length % 4 == 0) {
        auto kernel = symmetric ? sample_gaussian_f32x4_kernel<true> : sample_gaussian_f32x4_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream, reinterpret_cast<float4*>(out.data_ptr<float>()),
                           reinterpret_cast<const float4*>(mu.data_ptr<float>()),
                           reinterpret_cast<const float4*>(sigma.data_ptr<float>()), rows, length / 4, (uint64_t)seed,
                           seed_ptr, row_offset);
        return;
    }
    DISPATCH_FLOAT_T(out, "sample_gaussian", {
        auto kernel = symmetric ? sample_gaussian_kernel<T, true> : sample_gaussian_kernel<T, false>;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream, out.data_ptr<T>(), mu.data_ptr<T>(),
                           sigma.data_ptr<T>(), rows, length, (uint64_t)seed, seed_ptr, row_offset);
    });
}

void sample_gaussian(torch::Tensor out, torch::Tensor mu, torch::Tensor sigma, bool symmetric, int64_t seed,
                     int64_t row_offset) {
    sample_gaussian_impl(out, mu, sigma, symmetric, seed, nullptr, row_offset);
}

// Advance a device seed chain by one splitmix64 step (standalone entry for
// graph-safe consumers like the rollout kernels: bump, then launch with
// seed_buf — replays draw fresh episode seeds).
void bump_seed(torch::Tensor seed_buf) {
    hipLaunchKernelGGL(bump_seed_kernel, dim3(1), dim3(1), 0, at::cuda::getCurrentCUDAStream(),
                       device_i64_scalar(seed_buf, "seed_buf"));
}

// Graph-safe variant: the seed lives in `seed_buf` (int64 tensor of 1
// element) and is advanced ON DEVICE after sampling, so hipGraph replays
// draw fresh populations.
void sample_gaussian_graphsafe(torch::Tensor out, torch::Tensor mu, torch::Tensor sigma, bool symmetric,
                               torch::Tensor seed_buf) {
    sample_gaussian_impl(out, mu, sigma, symmetric, 0, device_i64_scalar(seed_buf, "seed_buf"));
    bump_seed(seed_buf);
}

// Apply x = mu + sigma*z from PRE-GENERATED standard normals (the noise
// was filled on a side stream, hidden behind evaluation / collectives;
// only this cheap bandwidth-bound affine pass sits on the critical path
// after the distribution update — SURVEY.md §2.8 P2 overlap).
// Symmetric: z has N/2 rows; out rows [0,N/2) = mu+sigma*z, mirrored below.
template <typename T, bool kSymmetric>
__global__ void affine_from_noise_kernel(T* __restrict__ out, const float* __restrict__ z,
                                         const T* __restrict__ mu, const T* __restrict__ sigma,
                                         int64_t rows, int64_t length) {
    const int64_t total = rows * length;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t col = e % length;
        const float m = static_cast<float>(mu[col]);
        const float s = static_cast<float>(sigma[col]);
        const float plus = fmaf(s, z[e], m);
        out[e] = static_cast<T>(plus);
        if (kSymmetric) out[e + total] = static_cast<T>(2.0f * m - plus);
    }
}

void affine_from_noise(torch::Tensor out, torch::Tensor z, torch::Tensor mu, torch::Tensor sigma, bool symmetric) {
    const int64_t rows = check_sampling_operands(out, mu, sigma, symmetric);
    const int64_t length = out.size(1);
    check_operand_as(z, "z", out, at::ScalarType::Float, rows * length);
    const int threads = 256;
    const int blocks = grid_for(rows * length, threads, 256 * 8);
    auto stream = at::cuda::getCurrentCUDAStream();
    DISPATCH_FLOAT_T(out, "affine_from_noise", {
        auto kernel = symmetric ? affine_from_noise_kernel<T, true> : affine_from_noise_kernel<T, false>;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream, out.data_ptr<T>(), z.data_ptr<float>(),
                           mu.data_ptr<T>(), sigma.data_ptr<T>(), rows, length);
    });
}

// ---------------------------------------------------------------------------
// K3: fused ES gradient reductions (N x L -> L), fp32 accumulation
// ---------------------------------------------------------------------------

enum class GradMode { kPlain, kSymmetric, kSnes };

template <typename T, GradMode kMode>
__global__ void es_grad_kernel(const T* __restrict__ x, const T* __restrict__ mu, const T* __restrict__ sigma,
                               const T* __restrict__ w, float* __restrict__ mu_grad, float* __restrict__ sigma_grad,
                               int64_t rows,  // = N (plain/snes) or N/2 directions (symmetric)
                               int64_t n_total, int64_t length, int row_chunks) {
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= length) return;
    const int chunk = blockIdx.y;
    const int64_t r0 = (rows * chunk) / row_chunks;
    const int64_t r1 = (rows * (chunk + 1)) / row_chunks;
    const float m = static_cast<float>(mu[col]);
    const float s = static_cast<float>(sigma[col]);
    float acc_mu = 0.0f, acc_sigma = 0.0f;
    for (int64_t r = r0; r < r1; ++r) {
        const float xv = static_cast<float>(x[r * length + col]);
        const float noise = xv - m;
        if (kMode == GradMode::kSymmetric) {
            const float wp = static_cast<float>(w[r]);
            const float wm = static_cast<float>(w[r + rows]);
            acc_mu = fmaf(0.5f * (wp - wm), noise, acc_mu);
            acc_sigma = fmaf(0.5f * (wp + wm), (noise * noise - s * s) / s, acc_sigma);
        } else if (kMode == GradMode::kPlain) {
            const float wv = static_cast<float>(w[r]);
            acc_mu = fmaf(wv, noise, acc_mu);
            acc_sigma = fmaf(wv, (noise * noise - s * s) / s, acc_sigma);
        } else {  // SNES: raw-noise sigma gradient
            const float wv = static_cast<float>(w[r]);
            const float raw = noise / s;
            acc_mu = fmaf(wv, noise, acc_mu);
            acc_sigma = fmaf(wv, raw * raw - 1.0f, acc_sigma);
        }
    }
    // per-chunk partial rows (summed by a deterministic torch reduction) —
    // float atomicAdd would make the gradient run-to-run order-dependent
    mu_grad[(int64_t)chunk * length + col] = acc_mu;
    sigma_grad[(int64_t)chunk * length + col] = acc_sigma;
}

template <GradMode kMode>
std::vector<torch::Tensor> es_grad_launch(torch::Tensor samples, torch::Tensor mu, torch::Tensor sigma,
                                          torch::Tensor weights) {
    check_primary(samples, "samples", 2);
    const int64_t n = samples.size(0), length = samples.size(1);
    check_operand(mu, "mu", samples, length);
    check_operand(sigma, "sigma", samples, length);
    check_operand(weights, "weights", samples, n);
    TORCH_CHECK(kMode != GradMode::kSymmetric || n % 2 == 0, "symmetric gradients need even popsize, got ", n);
    const int64_t rows = (kMode == GradMode::kSymmetric) ? n / 2 : n;
    auto opts = samples.options().dtype(torch::kFloat32);
    const int threads = 256;
    const int col_blocks = grid_for(length, threads);
    // fill the chip: >= ~1024 blocks total
    int row_chunks = 1;
    if (col_blocks < 1024) row_chunks = (int)std::min<int64_t>((1024 + col_blocks - 1) / col_blocks, std::max<int64_t>(rows / 8, 1));
    auto mu_grad = torch::empty({row_chunks, length}, opts);
    auto sigma_grad = torch::empty({row_chunks, length}, opts);
    auto stream = at::cuda::getCurrentCUDAStream();
    DISPATCH_FLOAT_T(samples, "es_gradients", {
        hipLaunchKernelGGL((es_grad_kernel<T, kMode>), dim3(col_blocks, row_chunks), dim3(threads), 0, stream,
                           samples.data_ptr<T>(), mu.data_ptr<T>(), sigma.data_ptr<T>(), weights.data_ptr<T>(),
                           mu_grad.data_ptr<float>(), sigma_grad.data_ptr<float>(), rows, n, length, row_chunks);
    });
    if (row_chunks > 1) {
        return {mu_grad.sum(0).to(samples.scalar_type()), sigma_grad.sum(0).to(samples.scalar_type())};
    }
    return {mu_grad.reshape({length}).to(samples.scalar_type()), sigma_grad.reshape({length}).to(samples.scalar_type())};
}

std::vector<torch::Tensor> es_gradients(torch::Tensor samples, torch::Tensor mu, torch::Tensor sigma,
                                        torch::Tensor weights, bool symmetric) {
    if (symmetric) return es_grad_launch<GradMode::kSymmetric>(samples, mu, sigma, weights);
    return es_grad_launch<GradMode::kPlain>(samples, mu, sigma, weights);
}

std::vector<torch::Tensor> snes_gradients(torch::Tensor samples, torch::Tensor mu, torch::Tensor sigma,
                                          torch::Tensor weights) {
    return es_grad_launch<GradMode::kSnes>(samples, mu, sigma, weights);
}

// ---------------------------------------------------------------------------
// K4: ClipUp (3 chained kernels, no host sync) and Adam
// ---------------------------------------------------------------------------

template <typename T>
__global__ void sumsq_kernel(const T* __restrict__ v, float* __restrict__ partials, int64_t n) {
    __shared__ float scratch[8];
    float acc = 0.0f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = static_cast<float>(v[i]);
        acc = fmaf(x, x, acc);
    }
    acc = block_reduce_sum<false>(acc, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// Deterministic per-block partial combine (float atomicAdd would make
// ClipUp's norms — and hence the whole trajectory — run-to-run
// order-dependent): one block sums `count` partials in fixed order.
__global__ void reduce_partials_kernel(const float* __restrict__ partials, float* __restrict__ out, int count) {
    __shared__ float scratch[8];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < count; i += blockDim.x) acc += partials[i];
    acc = block_reduce_sum<false>(acc, scratch);
    if (threadIdx.x == 0) *out = acc;
}

// velocity = momentum * velocity + grad * (step_size / ||grad||); also
// accumulates per-block ||velocity||^2 partials for the clip pass.
template <typename T>
__global__ void clipup_update_kernel(T* __restrict__ velocity, const T* __restrict__ grad,
                                     const float* __restrict__ gnorm_sq, float* __restrict__ vnorm_partials,
                                     float step_size, float momentum, int64_t n) {
    __shared__ float scratch[8];
    const float gnorm = sqrtf(fmaxf(*gnorm_sq, 1e-30f));
    const float scale = step_size / gnorm;
    float acc = 0.0f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = fmaf(momentum, static_cast<float>(velocity[i]), static_cast<float>(grad[i]) * scale);
        velocity[i] = static_cast<T>(v);
        acc = fmaf(v, v, acc);
    }
    acc = block_reduce_sum<false>(acc, scratch);
    if (threadIdx.x == 0) vnorm_partials[blockIdx.x] = acc;
}

template <typename T>
__global__ void clipup_clip_kernel(T* __restrict__ velocity, const float* __restrict__ vnorm_sq, float max_speed,
                                   int64_t n) {
    const float vnorm = sqrtf(fmaxf(*vnorm_sq, 1e-30f));
    const float scale = fminf(max_speed / vnorm, 1.0f);
    if (scale >= 1.0f) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        velocity[i] = static_cast<T>(static_cast<float>(velocity[i]) * scale);
    }
}

void clipup_step(torch::Tensor velocity, torch::Tensor grad, double step_size, double max_speed, double momentum) {
    check_primary(velocity, "velocity", 1);
    const int64_t n = velocity.numel();
    check_operand(grad, "grad", velocity, n);
    const int threads = 256;
    const int blocks = grid_for(n, threads, 1024);
    // [0] gnorm², [1] vnorm², [2..2+blocks) per-block partials
    auto scratch = torch::empty({2 + blocks}, velocity.options().dtype(torch::kFloat32));
    auto stream = at::cuda::getCurrentCUDAStream();
    DISPATCH_FLOAT_T(velocity, "clipup_step", {
        float* gnorm_sq = scratch.data_ptr<float>();
        float* vnorm_sq = gnorm_sq + 1;
        float* partials = gnorm_sq + 2;
        hipLaunchKernelGGL((sumsq_kernel<T>), dim3(blocks), dim3(threads), 0, stream, grad.data_ptr<T>(), partials, n);
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, partials, gnorm_sq, blocks);
        hipLaunchKernelGGL((clipup_update_kernel<T>), dim3(blocks), dim3(threads), 0, stream, velocity.data_ptr<T>(),
                           grad.data_ptr<T>(), gnorm_sq, partials, (float)step_size, (float)momentum, n);
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, partials, vnorm_sq, blocks);
        hipLaunchKernelGGL((clipup_clip_kernel<T>), dim3(blocks), dim3(threads), 0, stream, velocity.data_ptr<T>(),
                           vnorm_sq, (float)max_speed, n);
    });
}

// ---------------------------------------------------------------------------
// K4b: the whole distribution update of a separable Gaussian under ClipUp
// in ONE launch of one block: clipup_step on velocity, new_mu = mu +
// velocity, new_sigma = sigma + lr·sigma_grad held inside the stdev bounds
// (utils/misc.py modify_tensor with scalar bounds). Every value is what the
// chain of launches gives, bit for bit: elementwise steps are rounded one by
// one as separate kernels round them (contraction off; fmaf only where the
// chain has one), and the two norms are summed in clipup_step's own tree.
// ---------------------------------------------------------------------------

constexpr int kUpdateThreads = 1024;
// 256 virtual blocks of 256 threads: below grid_for's cap of 1024 blocks, so
// every virtual thread of clipup_step's kernels holds exactly one element
constexpr int64_t kUpdateMaxLength = 65536;

// Σ value(i)² over [0, n) in the order of sumsq_kernel / clipup_update_kernel
// followed by reduce_partials_kernel: virtual blocks of 256 threads, one
// element each, reduced by block_reduce_sum (four wave sums s0..s3 of a
// block combine as (s0 + s2) + (s1 + s3): lane 0 of a shfl_down tree over
// s0 s1 s2 s3 0 0 ..), then the partials, one per thread of a 256-thread
// block, by the same reduction. The 16 waves of this block walk the virtual
// blocks four at a time. `value` is called once for every i < n.
// wave_sums: [1024], tops: [4]; the result is returned to all threads.
template <typename F>
__device__ __forceinline__ float clipup_tree_sumsq(F value, int n, float* wave_sums, float* tops) {
    const int tid = threadIdx.x, lane = tid & (kWaveSize - 1), wave = tid / kWaveSize;
    const int vblocks = (n + 255) / 256;
    for (int base = 0; base < vblocks * 256; base += kUpdateThreads) {
        const int i = base + tid;
        const float x = (i < n) ? value(i) : 0.0f;
        const float w = wave_reduce_sum(fmaf(x, x, 0.0f));
        if (lane == 0) wave_sums[base / kWaveSize + wave] = w;
    }
    __syncthreads();
    if (tid < 256) {
        float part = 0.0f;
        if (tid < vblocks)
            part = (wave_sums[4 * tid] + wave_sums[4 * tid + 2]) + (wave_sums[4 * tid + 1] + wave_sums[4 * tid + 3]);
        part = wave_reduce_sum(part);
        if (lane == 0) tops[wave] = part;
    }
    __syncthreads();
    return (tops[0] + tops[2]) + (tops[1] + tops[3]);
}

// torch.maximum / torch.minimum: a NaN of either side comes through
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }

constexpr int kHasStdevMin = 1, kHasStdevMax = 2, kHasStdevMaxChange = 4;

__global__ __launch_bounds__(kUpdateThreads) void gaussian_clipup_update_kernel(
    const float* __restrict__ mu, const float* __restrict__ sigma, float* __restrict__ velocity,
    const float* __restrict__ mu_grad, const float* __restrict__ sigma_grad, float* __restrict__ new_mu,
    float* __restrict__ new_sigma, int n, float step_size, float momentum, float max_speed, float sigma_lr,
    float stdev_min, float stdev_max, float stdev_max_change, int bounds) {
#pragma clang fp contract(off)
    __shared__ float wave_sums[kUpdateThreads];
    __shared__ float tops[4];

    const float gnorm_sq = clipup_tree_sumsq([&](int i) { return mu_grad[i]; }, n, wave_sums, tops);
    const float gnorm = sqrtf(fmaxf(gnorm_sq, 1e-30f));
    const float scale = step_size / gnorm;
    const float vnorm_sq = clipup_tree_sumsq(
        [&](int i) {
            const float v = fmaf(momentum, velocity[i], mu_grad[i] * scale);
            velocity[i] = v;
            return v;
        },
        n, wave_sums, tops);
    const float vnorm = sqrtf(fmaxf(vnorm_sq, 1e-30f));
    const float clip = fminf(max_speed / vnorm, 1.0f);

    // element i was written above by this same thread
    for (int i = threadIdx.x; i < n; i += kUpdateThreads) {
        float v = velocity[i];
        if (!(clip >= 1.0f)) {
            v = v * clip;
            velocity[i] = v;
        }
        new_mu[i] = mu[i] + v;

        const float s = sigma[i];
        // torch.add(sigma, grad, alpha=lr) is one fma in torch's ROCm build
        float target = fmaf(sigma_lr, sigma_grad[i], s);
        if (bounds & kHasStdevMaxChange) {
            const float allowed = fabsf(s) * stdev_max_change;
            float lo = s - allowed;
            float hi = allowed + s;
            if ((bounds & kHasStdevMin) && lo == lo) lo = fmaxf(lo, stdev_min);
            if ((bounds & kHasStdevMax) && hi == hi) hi = fminf(hi, stdev_max);
            target = nan_min(nan_max(target, lo), hi);
        } else if (target == target) {
            if (bounds & kHasStdevMin) target = fmaxf(target, stdev_min);
            if (bounds & kHasStdevMax) target = fminf(target, stdev_max);
        }
        new_sigma[i] = target;
    }
}

std::vector<torch::Tensor> gaussian_clipup_update(torch::Tensor mu, torch::Tensor sigma, torch::Tensor velocity,
                                                  torch::Tensor mu_grad, torch::Tensor sigma_grad, double step_size,
                                                  double momentum, double max_speed, double sigma_lr,
                                                  c10::optional<double> stdev_min, c10::optional<double> stdev_max,
                                                  c10::optional<double> stdev_max_change) {
    check_primary(mu, "mu", 1);
    TORCH_CHECK(mu.scalar_type() == torch::kFloat32, "gaussian_clipup_update expects float32, got ", mu.scalar_type());
    const int64_t n = mu.numel();
    TORCH_CHECK(n >= 1 && n <= kUpdateMaxLength, "gaussian_clipup_update supports 1 <= L <= ", kUpdateMaxLength,
                ", got ", n);
    check_operand(sigma, "sigma", mu, n);
    check_operand(velocity, "velocity", mu, n);
    check_operand(mu_grad, "mu_grad", mu, n);
    check_operand(sigma_grad, "sigma_grad", mu, n);
    auto new_mu = torch::empty_like(mu);
    auto new_sigma = torch::empty_like(sigma);
    const int bounds = (stdev_min ? kHasStdevMin : 0) | (stdev_max ? kHasStdevMax : 0) |
                       (stdev_max_change ? kHasStdevMaxChange : 0);
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(gaussian_clipup_update_kernel, dim3(1), dim3(kUpdateThreads), 0, stream, mu.data_ptr<float>(),
                       sigma.data_ptr<float>(), velocity.data_ptr<float>(), mu_grad.data_ptr<float>(),
                       sigma_grad.data_ptr<float>(), new_mu.data_ptr<float>(), new_sigma.data_ptr<float>(), (int)n,
                       (float)step_size, (float)momentum, (float)max_speed, (float)sigma_lr,
                       (float)stdev_min.value_or(0.0), (float)stdev_max.value_or(0.0),
                       (float)stdev_max_change.value_or(0.0), bounds);
    return {new_mu, new_sigma};
}

int64_t gaussian_clipup_update_max_length() { return kUpdateMaxLength; }

// One element of the Adam ascent step, shared by both kernels below.
template <typename T>
__device__ __forceinline__ void adam_element(T* __restrict__ step_out, const T* __restrict__ grad, T* __restrict__ m,
                                             T* __restrict__ v, int64_t i, float stepsize, float beta1, float beta2,
                                             float epsilon, float bias1, float bias2) {
    const float g = static_cast<float>(grad[i]);
    const float m_new = fmaf(beta1, static_cast<float>(m[i]), (1.0f - beta1) * g);
    const float v_new = fmaf(beta2, static_cast<float>(v[i]), (1.0f - beta2) * g * g);
    m[i] = static_cast<T>(m_new);
    v[i] = static_cast<T>(v_new);
    step_out[i] = static_cast<T>(stepsize * (m_new / bias1) / (sqrtf(v_new / bias2) + epsilon));
}

// Bias corrections computed on the HOST (host powf): the two kernels stay
// separate because the plain path's bits depend on which powf ran.
template <typename T>
__global__ void adam_kernel(T* __restrict__ step_out, const T* __restrict__ grad, T* __restrict__ m,
                            T* __restrict__ v, float stepsize, float beta1, float beta2, float epsilon,
                            float bias1, float bias2, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adam_element(step_out, grad, m, v, i, stepsize, beta1, beta2, epsilon, bias1, bias2);
}

// Graph-safe Adam: the step count lives in a device buffer and is
// advanced ON DEVICE, so hipGraph replays apply the correct bias
// correction each generation (a by-value step count would freeze it).
template <typename T>
__global__ void adam_graphsafe_kernel(T* __restrict__ step_out, const T* __restrict__ grad, T* __restrict__ m,
                                      T* __restrict__ v, const long long* __restrict__ t_buf, float stepsize,
                                      float beta1, float beta2, float epsilon, int64_t n) {
    const float t = (float)(*t_buf + 1);
    const float bias1 = 1.0f - powf(beta1, t);
    const float bias2 = 1.0f - powf(beta2, t);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adam_element(step_out, grad, m, v, i, stepsize, beta1, beta2, epsilon, bias1, bias2);
}

__global__ void bump_step_kernel(long long* t_buf) { *t_buf += 1; }

// Operand checks of both Adam entry points; returns the element count.
static int64_t check_adam_operands(const torch::Tensor& step_out, const torch::Tensor& grad, const torch::Tensor& m,
                                   const torch::Tensor& v) {
    check_primary(step_out, "step_out", 1);
    const int64_t n = step_out.numel();
    check_operand(grad, "grad", step_out, n);
    check_operand(m, "m", step_out, n);
    check_operand(v, "v", step_out, n);
    return n;
}

void adam_step_graphsafe(torch::Tensor step_out, torch::Tensor grad, torch::Tensor m, torch::Tensor v,
                         torch::Tensor t_buf, double stepsize, double beta1, double beta2, double epsilon) {
    const int64_t n = check_adam_operands(step_out, grad, m, v);
    auto* t_ptr = reinterpret_cast<long long*>(device_i64_scalar(t_buf, "t_buf"));
    const int threads = 256;
    const int blocks = grid_for(n, threads, 2048);
    auto stream = at::cuda::getCurrentCUDAStream();
    DISPATCH_FLOAT_T(step_out, "adam_graphsafe", {
        hipLaunchKernelGGL((adam_graphsafe_kernel<T>), dim3(blocks), dim3(threads), 0, stream, step_out.data_ptr<T>(),
                           grad.data_ptr<T>(), m.data_ptr<T>(), v.data_ptr<T>(), t_ptr, (float)stepsize,
                           (float)beta1, (float)beta2, (float)epsilon, n);
    });
    hipLaunchKernelGGL(bump_step_kernel, dim3(1), dim3(1), 0, stream, t_ptr);
}

void adam_step(torch::Tensor step_out, torch::Tensor grad, torch::Tensor m, torch::Tensor v, int64_t step_count,
               double stepsize, double beta1, double beta2, double epsilon) {
    const int64_t n = check_adam_operands(step_out, grad, m, v);
    const int threads = 256;
    const int blocks = grid_for(n, threads, 2048);
    const float bias1 = 1.0f - powf((float)beta1, (float)step_count);
    const float bias2 = 1.0f - powf((float)beta2, (float)step_count);
    auto stream = at::cuda::getCurrentCUDAStream();
    DISPATCH_FLOAT_T(step_out, "adam_step", {
        hipLaunchKernelGGL((adam_kernel<T>), dim3(blocks), dim3(threads), 0, stream, step_out.data_ptr<T>(),
                           grad.data_ptr<T>(), m.data_ptr<T>(), v.data_ptr<T>(), (float)stepsize, (float)beta1,
                           (float)beta2, (float)epsilon, bias1, bias2, n);
    });
}

// ---------------------------------------------------------------------------
// K2: fused fitness ranking -> utility map (reference
// tools/ranking.py:24-216). One launch replaces the torch chain
// (rocPRIM radix sort + scatter + 3-4 elementwise maps): a single-block
// bitonic sort (N <= 8192 padded to a power of two p with +inf) followed by
// the utility map written back through the sorted index payload.
// method: 0 = centered (rank/(n-1) - 0.5), 1 = linear (rank/(n-1)),
//         2 = nes (log-utilities, normalized to sum to ~0).
//
// The comparator network is the serial one — for k = 2, 4 .. p, for
// j = k/2 .. 1: compare-exchange (i, i^j), ascending where (i & k) == 0 —
// and ties stay where the network leaves them, so its step order and swap
// predicate fix the result bit for bit. Only the place of the data varies:
// thread t of the 1024 holds positions [t·E, (t+1)·E), E = max(1, p/1024),
// as (key, index) pairs in registers. A step with j < E exchanges inside a
// thread, one with E <= j < 64·E between two lanes of a wave (no barrier),
// and only j >= 64·E goes through LDS behind barriers: 10 of the 78 steps at
// p = 4096. In the two-thread forms both threads evaluate the predicate of
// the lower position on the same two keys and so agree.
// ---------------------------------------------------------------------------

constexpr int kRankThreads = 1024;

// The swap predicate on fp32 keys a (lower position) and b, NaN-robust:
// NaNs order last so they rank as best-key (matches torch argsort's
// NaN-is-largest behavior), and on a tie nothing moves:
//   ascending:  b < a || (isnan(a) && !isnan(b))
//   descending: a < b || (isnan(b) && !isnan(a))
// It is evaluated on order keys: rank_order_key maps fp32 to int32 such that
// the ascending predicate is exactly key(b) < key(a) and the descending one
// key(a) < key(b) — monotone on the non-NaN values, -0 and +0 onto one key
// (neither is < the other), every NaN onto INT_MAX (above +inf's key, and
// no NaN before another). One integer compare then decides a
// compare-exchange; on one CU the predicate's ~20 float instructions per
// evaluation were most of the kernel's time.
__device__ __forceinline__ int rank_order_key(float x) {
    if (isnan(x)) return INT_MAX;
    const int bits = __float_as_int(x);
    return bits >= 0 ? bits : -(bits & 0x7fffffff);
}

// This thread's side of the compare-exchange with the position held by a
// partner thread. `lower_is_up` = (this thread holds the lower position) ==
// (the pair sorts ascending): then it takes the partner's pair iff the
// partner's key is smaller, otherwise iff it is larger.
__device__ __forceinline__ void rank_exchange(int& key, int& idx, int other_key, int other_idx, bool lower_is_up) {
    if (lower_is_up ? (other_key < key) : (key < other_key)) {
        key = other_key;
        idx = other_idx;
    }
}

template <int E>
__global__ __launch_bounds__(kRankThreads) void fused_rank_kernel(const float* __restrict__ fit,
                                                                  float* __restrict__ out, int n, int p, int method,
                                                                  bool higher_better) {
    extern __shared__ unsigned char rank_lds[];
    constexpr int kSlots = E * kRankThreads;  // >= p
    float* keys = reinterpret_cast<float*>(rank_lds);
    int* idx = reinterpret_cast<int*>(keys + kSlots);
    float* scratch = reinterpret_cast<float*>(idx + kSlots);  // [32] for the nes sum
    int* order_keys = reinterpret_cast<int*>(keys);           // the sort's use of the key slots

    const int tid = threadIdx.x;
    int key[E];
    int id[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        key[e] = rank_order_key((i < n) ? (higher_better ? fit[i] : -fit[i]) : INFINITY);
        id[e] = i;
    }
    // bitonic sort ascending: position 0 = worst
    for (int k = 2; k <= p; k <<= 1) {
        int j = k >> 1;
        // with a partner in another thread j >= E, so k > E and the
        // direction bit (i & k) is the same for all E positions of a thread
        const bool up = ((tid * E) & k) == 0;
        // partner in another wave: through LDS, laid out [e][thread] so
        // that lanes touch consecutive banks
        for (; j >= 64 * E; j >>= 1) {
            const int m = j / E;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                order_keys[e * kRankThreads + tid] = key[e];
                idx[e * kRankThreads + tid] = id[e];
            }
            __syncthreads();
            int other_key[E];
            int other_id[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                other_key[e] = order_keys[e * kRankThreads + (tid ^ m)];
                other_id[e] = idx[e * kRankThreads + (tid ^ m)];
            }
            __syncthreads();
            const bool lower_is_up = ((tid & m) == 0) == up;
#pragma unroll
            for (int e = 0; e < E; ++e) rank_exchange(key[e], id[e], other_key[e], other_id[e], lower_is_up);
        }
        // partner in another lane of this wave
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            if (m * E < k) {
                const bool lower_is_up = ((tid & m) == 0) == up;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int other_key = __shfl_xor(key[e], m, 64);
                    const int other_id = __shfl_xor(id[e], m, 64);
                    rank_exchange(key[e], id[e], other_key, other_id, lower_is_up);
                }
            }
        }
        // partner in this thread
#pragma unroll
        for (int jj = E / 2; jj > 0; jj >>= 1) {
            if (jj < k) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & jj) == 0) {
                        const int a = key[e], b = key[e | jj];
                        if ((((tid * E + e) & k) == 0) ? (b < a) : (a < b)) {
                            key[e] = b; key[e | jj] = a;
                            const int t = id[e]; id[e] = id[e | jj]; id[e | jj] = t;
                        }
                    }
                }
            }
        }
    }
    // the sorted index payload back to LDS in position order for the utility
    // map (the map reads no key; nes reuses the key slots for its utilities)
#pragma unroll
    for (int e = 0; e < E; ++e) idx[tid * E + e] = id[e];
    __syncthreads();
    // a pad slot (index >= n) can sort in front of real ones only for
    // non-finite fitness; it has no output element
    if (method == 2) {
        // NES log-utilities need their global sum before the final map
        float partial = 0.0f;
        for (int i = tid; i < n; i += blockDim.x) {
            const float rank_from_best = (float)(n - i);
            const float u = fmaxf(__logf((float)n / 2.0f + 1.0f) - __logf(rank_from_best), 0.0f);
            keys[i] = u;  // reuse the key slot for the raw utility
            partial += u;
        }
        __syncthreads();
        // block sum (1024 threads -> 32 warp partials -> one value)
        const int lane = tid & 63, wave = tid >> 6;
        for (int off = 32; off > 0; off >>= 1) partial += __shfl_down(partial, off, 64);
        if (lane == 0) scratch[wave] = partial;
        __syncthreads();
        if (tid == 0) {
            float total = 0.0f;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += scratch[w];
            scratch[0] = total;
        }
        __syncthreads();
        const float denom = scratch[0];
        const float inv_n = 1.0f / (float)n;
        for (int i = tid; i < n; i += blockDim.x)
            if (idx[i] < n) out[idx[i]] = keys[i] / denom - inv_n;
        return;
    }
    const float inv = (n > 1) ? 1.0f / (float)(n - 1) : 0.0f;
    for (int i = tid; i < n; i += blockDim.x) {
        const float r = (float)i;
        if (idx[i] < n) out[idx[i]] = (method == 0) ? (r * inv - 0.5f) : (r * inv);
    }
}

template <int E>
static void fused_rank_launch(const torch::Tensor& fit, torch::Tensor& out, int n, int p, int method,
                              bool higher_better) {
    constexpr size_t lds = (size_t)E * kRankThreads * 8 + 32 * 4;
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        allow_max_dynamic_lds(reinterpret_cast<const void*>(&fused_rank_kernel<E>));
        attr_set = true;
    }
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL((fused_rank_kernel<E>), dim3(1), dim3(kRankThreads), lds, stream, fit.data_ptr<float>(),
                       out.data_ptr<float>(), n, p, method, higher_better);
}

torch::Tensor fused_rank(torch::Tensor fitnesses, int64_t method, bool higher_better) {
    TORCH_CHECK(fitnesses.is_cuda() && fitnesses.dim() == 1, "fused_rank expects a 1-D ROCm tensor");
    auto fit = fitnesses.to(torch::kFloat32).contiguous();
    const int n = (int)fit.size(0);
    TORCH_CHECK(n >= 1 && n <= 8192, "fused_rank supports 1 <= n <= 8192");
    int p = 1;
    while (p < n) p <<= 1;
    auto out = torch::empty({n}, fit.options());
    switch (std::max(1, p / kRankThreads)) {
        case 1: fused_rank_launch<1>(fit, out, n, p, (int)method, higher_better); break;
        case 2: fused_rank_launch<2>(fit, out, n, p, (int)method, higher_better); break;
        case 4: fused_rank_launch<4>(fit, out, n, p, (int)method, higher_better); break;
        default: fused_rank_launch<8>(fit, out, n, p, (int)method, higher_better); break;
    }
    return out;
}

}  // namespace ea
