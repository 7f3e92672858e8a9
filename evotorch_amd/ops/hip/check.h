// Host-side operand checks and launch helpers shared by every launcher of
// the extension. A kernel reads exactly what its launcher passed: a short,
// strided, wrongly typed or host-resident operand is a GPU fault or silent
// garbage, so every tensor is checked here BEFORE anything is allocated or
// launched. No device code in this header.
#pragma once
#include <hip/hip_runtime.h>
#include <ATen/core/Tensor.h>
#include <c10/util/Exception.h>

#include <algorithm>
#include <climits>

namespace ea {

inline void check_same_device(const at::Tensor& t, const char* name, const at::Tensor& like) {
    TORCH_CHECK(t.device() == like.device(), name, " must be on ", like.device(), ", got ", t.device());
}

// The tensor that fixes a launch's device, dtype and sizes.
inline void check_primary(const at::Tensor& t, const char* name, int64_t dim) {
    TORCH_CHECK(t.is_cuda(), name, " must be a ROCm tensor, got ", t.device());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.dim() == dim, name, " must be ", dim, "-D, got ", t.dim(), "-D");
}

// Any other operand: on `like`'s device, of the given dtype, dense, and of
// EXACTLY `numel` elements.
inline void check_operand_as(const at::Tensor& t, const char* name, const at::Tensor& like,
                             at::ScalarType dtype, int64_t numel) {
    check_same_device(t, name, like);
    TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.numel() == numel, name, " must have ", numel, " elements, got ", t.numel());
}

inline void check_operand(const at::Tensor& t, const char* name, const at::Tensor& like, int64_t numel) {
    check_operand_as(t, name, like, like.scalar_type(), numel);
}

// Device-resident int64 scalar (hipGraph-safe seed chains and step counts).
inline unsigned long long* device_i64_scalar(const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::ScalarType::Long && t.numel() >= 1, name,
                " must be a device int64 scalar");
    return reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>());
}

// Blocks of `threads` covering n elements, at most `cap` (grid-stride
// kernels saturate the chip well below one block per 256 elements).
inline int grid_for(int64_t n, int threads, int64_t cap = INT_MAX) {
    return (int)std::min<int64_t>((n + threads - 1) / threads, cap);
}

// Kernels whose dynamic LDS exceeds the 64 KB default need the limit raised
// once per kernel function.
inline void allow_max_dynamic_lds(const void* kernel) {
    const hipError_t err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    TORCH_CHECK(err == hipSuccess, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: ", hipGetErrorString(err));
}

}  // namespace ea
