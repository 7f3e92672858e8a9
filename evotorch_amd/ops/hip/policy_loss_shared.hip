// K17: the entry point of the fused shared-minibatch loss. The kernels are
// the kLoss instantiations of K14 (policy_forward_shared.hip, fp32 MFMA) and
// K15 (policy_forward_shared_bf16.hip, bf16 MFMA); the loss phase they end
// with is policy_loss.h. Here: the operand checks, the tile count, and the
// one reduction over the tile axis when a member has more than one tile.
//
// One block per (member, batch tile) writes partial[m][tile], the tile's sum
// already divided by the divisor (B * D_last, or the number of targets that
// are not ignored). With one tile (B <= BT) that is loss[m] and the launch is
// the only one; otherwise one at::sum_out over the tile axis follows, in an
// order that is a fixed function of the tile count.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <limits>

#include "check.h"
#include "policy_common.h"
#include "policy_loss.h"

namespace ea {

static void check_loss_kind(int64_t loss_kind) {
    TORCH_CHECK(loss_kind == kLossMse || loss_kind == kLossCrossEntropy,
                "loss_kind must be 0 (MSE) or 1 (cross-entropy), got ", loss_kind);
}

// Rows per batch tile the loss kernel takes for these widths (host only).
int64_t population_mlp_loss_shared_batch_tile(std::vector<int64_t> widths, bool bf16) {
    int width[kMaxLayers + 1], act[kMaxLayers];
    const std::vector<int64_t> identity(widths.empty() ? 0 : widths.size() - 1, kActIdentity);
    check_dense_stack(widths, identity, false, width, act);
    const int layers = (int)widths.size() - 1;
    return bf16 ? bf16_loss_batch_tile(width, layers) : shared_loss_batch_tile(width, layers);
}

torch::Tensor population_mlp_loss_shared(torch::Tensor params, torch::Tensor x, torch::Tensor y,
                                         std::vector<int64_t> widths, std::vector<int64_t> activations, bool has_bias,
                                         int64_t loss_kind, bool bf16) {
    check_primary(params, "params", 2);
    TORCH_CHECK(params.scalar_type() == torch::kFloat32, "params must be float32, got ", params.scalar_type());
    SharedForwardArgs args{};
    const int64_t expected = check_dense_stack(widths, activations, has_bias, args.width, args.act);
    const int64_t layers = (int64_t)widths.size() - 1;
    const int64_t n = params.size(0), L = params.size(1);
    TORCH_CHECK(L == expected, "params must hold ", expected, " values per member for this stack, got L = ", L);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == widths[0], "x must be 2-D (B, ", widths[0], "), got ", x.sizes());
    const int64_t B = x.size(0), D = widths[layers];
    check_operand(x, "x", params, B * widths[0]);
    check_loss_kind(loss_kind);
    if (loss_kind == kLossMse) {
        check_operand(y, "y", params, B * D);
        TORCH_CHECK(y.dim() == 2 && y.size(0) == B, "y must be 2-D (", B, ", ", D, ") for MSE, got ", y.sizes());
    } else {
        check_operand_as(y, "y", params, at::ScalarType::Long, B);
        TORCH_CHECK(y.dim() == 1, "y must be 1-D (", B, ",) class indices for cross-entropy, got ", y.sizes());
    }
    const int bt = bf16 ? bf16_loss_batch_tile(args.width, (int)layers) : shared_loss_batch_tile(args.width, (int)layers);
    const int64_t tiles = (B + bt - 1) / bt;
    TORCH_CHECK(B <= INT_MAX - 64, "x: too many rows (", B, ")");
    TORCH_CHECK(n * tiles <= INT_MAX - kXcds, "params, x: too many (member, batch tile) blocks (", n * tiles, ")");

    if (n == 0) return torch::empty({0}, params.options());
    if (B == 0) return torch::full({n}, std::numeric_limits<float>::quiet_NaN(), params.options());  // the mean of nothing
    torch::Tensor partial = torch::empty({n, tiles}, params.options());
    args.params = params.data_ptr<float>();
    args.x = x.data_ptr<float>();
    args.out = nullptr;
    args.B = (int)B;
    args.tiles = (int)tiles;
    args.blocks = (int)(n * tiles);
    args.L = (long)L;
    args.layers = (int)layers;
    args.has_bias = has_bias ? 1 : 0;
    SharedLossArgs largs{};
    if (loss_kind == kLossMse) {
        largs.y_mse = y.data_ptr<float>();
    } else {
        largs.y_ce = reinterpret_cast<const long long*>(y.data_ptr<int64_t>());
    }
    largs.loss = partial.data_ptr<float>();
    largs.kind = (int)loss_kind;
    largs.group = shared_loss_group((int)D);
    auto stream = at::cuda::getCurrentCUDAStream();
    if (bf16) {
        launch_shared_loss_bf16(args, largs, bt, stream);
    } else {
        launch_shared_loss(args, largs, bt, stream);
    }
    if (tiles == 1) return partial.view({n});
    torch::Tensor loss = torch::empty({n}, params.options());
    at::sum_out(loss, partial, {1});
    return loss;
}

}  // namespace ea
