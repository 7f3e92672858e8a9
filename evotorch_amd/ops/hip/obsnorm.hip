// K12: observation-normalization statistics on the stream, one launch each
// (neuroevolution/runningnorm.py). Both kernels give RunningNorm's own torch
// chains bit for bit: every elementwise step is rounded by itself, as the
// separate torch kernels round it (contraction off), divisions are true
// divisions, and a NaN passes through a clamp as torch.clamp passes it.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "check.h"

namespace ea {

// RunningNorm.mean / .stdev:
//   c     = clamp(count, min=1) in fp64, then to fp32
//   mean  = sum / c
//   stdev = sqrt(clamp(sumsq / c - mean * mean, min=min_variance))
// written to out_mean[0 : O) and out_std[0 : O).
__global__ void obsnorm_pack_kernel(const double* __restrict__ count, const float* __restrict__ sum,
                                    const float* __restrict__ sumsq, float min_variance,
                                    float* __restrict__ out_mean, float* __restrict__ out_std, int n) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double c64 = *count;
    const float c = static_cast<float>(c64 != c64 ? c64 : fmax(c64, 1.0));
    const float mean = sum[i] / c;
    const float mean_sq = mean * mean;
    const float var = sumsq[i] / c - mean_sq;
    const float floored = var != var ? var : fmaxf(var, min_variance);
    out_mean[i] = mean;
    out_std[i] = sqrtf(floored);
}

void obsnorm_pack(torch::Tensor count, torch::Tensor sum, torch::Tensor sumsq, double min_variance,
                  torch::Tensor blob, int64_t offset) {
    check_primary(blob, "blob", 1);
    TORCH_CHECK(blob.scalar_type() == torch::kFloat32, "blob must be float32, got ", blob.scalar_type());
    const int64_t n = sum.numel();
    TORCH_CHECK(n >= 1 && n <= INT_MAX, "obsnorm_pack: bad statistics length ", n);
    check_operand(sum, "sum", blob, n);
    check_operand(sumsq, "sumsq", blob, n);
    check_operand_as(count, "count", blob, torch::kFloat64, 1);
    TORCH_CHECK(offset >= 0 && offset + 2 * n <= blob.numel(), "obsnorm_pack: [offset, offset + 2*", n,
                ") does not fit a blob of ", blob.numel(), " elements (offset ", offset, ")");
    const int threads = 256;
    auto stream = at::cuda::getCurrentCUDAStream();
    float* tail = blob.data_ptr<float>() + offset;
    hipLaunchKernelGGL(obsnorm_pack_kernel, dim3(grid_for(n, threads)), dim3(threads), 0, stream,
                       count.data_ptr<double>(), sum.data_ptr<float>(), sumsq.data_ptr<float>(), (float)min_variance,
                       tail, tail + n, (int)n);
}

// RunningNorm.update((c, s, ss)): count += c (fp64); sum += s; sumsq += ss.
// c comes from the host, or from a 0-dim device tensor (fp32 or fp64) that
// is read on the device: no host sync.
__global__ void obsnorm_merge_kernel(double* __restrict__ count, float* __restrict__ sum, float* __restrict__ sumsq,
                                     double c_host, const float* __restrict__ c_f32,
                                     const double* __restrict__ c_f64, const float* __restrict__ s,
                                     const float* __restrict__ ss, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        const double c = c_f64 ? *c_f64 : (c_f32 ? static_cast<double>(*c_f32) : c_host);
        *count += c;
    }
    if (i >= n) return;
    sum[i] += s[i];
    sumsq[i] += ss[i];
}

void obsnorm_merge(torch::Tensor count, torch::Tensor sum, torch::Tensor sumsq, double c_host,
                   c10::optional<torch::Tensor> c_device, torch::Tensor s, torch::Tensor ss) {
    TORCH_CHECK(sum.is_cuda() && sum.is_contiguous(), "sum must be a contiguous ROCm tensor");
    TORCH_CHECK(sum.scalar_type() == torch::kFloat32, "sum must be float32, got ", sum.scalar_type());
    const int64_t n = sum.numel();
    TORCH_CHECK(n >= 1 && n <= INT_MAX, "obsnorm_merge: bad statistics length ", n);
    check_operand(sumsq, "sumsq", sum, n);
    check_operand(s, "s", sum, n);
    check_operand(ss, "ss", sum, n);
    check_operand_as(count, "count", sum, torch::kFloat64, 1);
    const float* c_f32 = nullptr;
    const double* c_f64 = nullptr;
    if (c_device.has_value()) {
        const torch::Tensor& c = *c_device;
        check_same_device(c, "c", sum);
        TORCH_CHECK(c.numel() == 1, "c must hold one element, got ", c.numel());
        if (c.scalar_type() == torch::kFloat64) {
            c_f64 = c.data_ptr<double>();
        } else {
            TORCH_CHECK(c.scalar_type() == torch::kFloat32, "c must be float32 or float64, got ", c.scalar_type());
            c_f32 = c.data_ptr<float>();
        }
    }
    const int threads = 256;
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(obsnorm_merge_kernel, dim3(grid_for(n, threads)), dim3(threads), 0, stream,
                       count.data_ptr<double>(), sum.data_ptr<float>(), sumsq.data_ptr<float>(), c_host, c_f32, c_f64,
                       s.data_ptr<float>(), ss.data_ptr<float>(), (int)n);
}

}  // namespace ea
