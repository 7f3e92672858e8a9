"""K15 `ops.population_forward_shared_bf16` / `_C.population_mlp_forward_shared_bf16`:
K14's shared-minibatch forward with weights, x and hidden activations rounded
to bf16, one launch on bf16 MFMA (ops/hip/policy_forward_shared_bf16.hip), and
its routing from `forward_shared(..., precision="bf16")` and
`SupervisedNE(..., forward_precision="bf16")`.

Numerics are held against the op's own eager chain in float64 on the CPU."""

import pytest
import torch
from torch import nn

from evotorch_amd import ops
from evotorch_amd.core import SolutionBatch
from evotorch_amd.models.functional import make_functional_module
from evotorch_amd.neuroevolution import SupervisedNE

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu(test):
    return pytest.mark.gpu(requires_gpu(test))


ID, TANH, RELU = 0, 1, 2

# name -> (widths, activations, has_bias)
STACKS = {
    "k3_identity": ([3, 2], [ID], True),  # K < 8, N < 16
    "odd_tanh": ([5, 17, 3], [TANH, ID], True),  # N one past a column tile
    "three_layers": ([33, 64, 65, 1], [RELU, TANH, ID], True),  # K = 33, 65 cross a 32-step by one; N = 1
    "no_bias": ([20, 9, 4], [TANH, RELU], False),
    "longest_k": ([1024, 8], [ID], True),
    "widest_lds": ([16, 1024, 16], [TANH, ID], True),
    "mnist": ([784, 128, 10], [TANH, ID], True),  # the stack the kernel exists for
}
SIZES = [(1, 1), (3, 17), (2, 64), (5, 130)]


def _inputs(widths, has_bias, n, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = sum(j * k + (j if has_bias else 0) for k, j in zip(widths[:-1], widths[1:]))
    return 0.3 * torch.randn(n, L, generator=g), torch.randn(B, widths[0], generator=g)


@gpu
@pytest.mark.parametrize("n,B", SIZES)
@pytest.mark.parametrize("stack", list(STACKS))
def test_numerics(stack, n, B):
    """|out - exact| <= 1e-5 (1 + |exact|), exact the eager chain in float64. With hidden layers a
    hidden value next to a bf16 rounding tie may round the other way than in float64, which moves
    its (member, row)'s outputs by up to a bf16 ulp of the value (2^-8 relative, on at most ~8)
    times a weight (at most ~1.3): up to 5 % of the outputs may miss the bound and must stay within
    5e-2 (1 + |exact|)."""
    widths, activations, has_bias = STACKS[stack]
    params, x = _inputs(widths, has_bias, n, B)
    exact = ops.population_forward_shared_bf16(params.double(), x.double(), widths, activations, has_bias)
    out = ops.population_forward_shared_bf16(params.cuda(), x.cuda(), widths, activations, has_bias).cpu()
    assert out.shape == (n, B, widths[-1]) and out.dtype == torch.float32
    err = (out.double() - exact).abs()
    outliers = err > 1e-5 * (1 + exact.abs())
    print(f"{stack} n={n} B={B}: max|err|={err.max().item():.3e} outliers={outliers.float().mean().item():.4f}")
    assert outliers.float().mean().item() <= (0.05 if len(widths) > 2 else 0.0)
    assert (err <= 5e-2 * (1 + exact.abs())).all()


@gpu
@pytest.mark.parametrize("stack", ["three_layers", "mnist"])
def test_output_is_independent_of_the_launch(stack):
    widths, activations, has_bias = STACKS[stack]
    params, x = (t.cuda() for t in _inputs(widths, has_bias, 5, 130, seed=1))
    whole = ops.population_forward_shared_bf16(params, x, widths, activations, has_bias)
    alone = ops.population_forward_shared_bf16(params[2:3], x[70:71], widths, activations, has_bias)
    assert torch.equal(whole[2, 70], alone[0, 0])
    assert torch.equal(whole[:, :17], ops.population_forward_shared_bf16(params, x[:17], widths, activations, has_bias))


@gpu
def test_routing():
    g = torch.Generator().manual_seed(4)
    X, Y = torch.randn(96, 8, generator=g), torch.randn(96, 1, generator=g)
    net = nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 1))
    values = (0.3 * torch.randn(7, 8 * 16 + 16 + 16 + 1, generator=g)).cuda()

    def problem():  # same seed: the CPU DataLoader generator draws the same minibatch
        return SupervisedNE(torch.utils.data.TensorDataset(X, Y), net, nn.functional.mse_loss, minibatch_size=32,
                            device="cuda:0", seed=3, forward_precision="bf16")

    evaluated = problem()
    batch = SolutionBatch(evaluated, popsize=7)
    batch.access_values()[:] = values.to(batch.device)
    evaluated.evaluate(batch)
    xb, yb = (t.cuda() for t in next(iter(problem().make_dataloader())))
    preds = ops.population_forward_shared_bf16(values, xb, [8, 16, 1], [TANH, ID], True)
    routed = torch.func.vmap(lambda p: nn.functional.mse_loss(p, yb))(preds)
    assert torch.equal(torch.Tensor.as_subclass(batch.evals[:, 0], torch.Tensor).cuda(), routed)

    # a stack too wide for K14's routing rule: bf16 takes the new op, the default keeps the vmap line
    fmodule = make_functional_module(nn.Linear(784, 4))
    x = torch.randn(6, 784, generator=g).cuda()
    params = (0.3 * torch.randn(5, fmodule.parameter_count, generator=g)).cuda()
    bf16 = ops.population_forward_shared_bf16(params, x, [784, 4], [ID], True)
    assert torch.equal(fmodule.forward_shared(params, x, precision="bf16"), bf16)
    vmapped = torch.func.vmap(fmodule._single, in_dims=(0, None))(params, x)
    assert torch.equal(fmodule.forward_shared(params, x), vmapped) and not torch.equal(vmapped, bf16)
    with pytest.raises(ValueError, match="precision"):
        fmodule.forward_shared(params, x, precision="fp8")


W, A = [6, 4, 3], [TANH, ID]
L = 6 * 4 + 4 + 4 * 3 + 3
# name -> (what the error names, params, x, widths, activations); x is moved to the device by the test
REJECTED = {
    "params_host": ("params", lambda: torch.ones(2, L), lambda: torch.ones(5, 6), W, A),
    "params_fp64": ("params", lambda: torch.ones(2, L, dtype=torch.float64).cuda(), lambda: torch.ones(5, 6), W, A),
    "params_strided": ("params", lambda: torch.ones(2, 2 * L).cuda()[:, ::2], lambda: torch.ones(5, 6), W, A),
    "L_short": (f"{L} values per member.*{L - 1}", lambda: torch.ones(2, L - 1).cuda(), lambda: torch.ones(5, 6), W, A),
    "x_width": ("x must be 2-D", lambda: torch.ones(2, L).cuda(), lambda: torch.ones(5, 7), W, A),
    "x_3d": ("x must be 2-D", lambda: torch.ones(2, L).cuda(), lambda: torch.ones(5, 1, 6), W, A),
    "width_1025": ("widths", lambda: torch.ones(2, 1025 * 8).cuda(), lambda: torch.ones(5, 1025), [1025, 7], [ID]),
}


@gpu
@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_operand(case):
    import evotorch_amd._C as C

    names, params, x, widths, activations = REJECTED[case]
    with pytest.raises(RuntimeError, match=names):
        C.population_mlp_forward_shared_bf16(params(), x().cuda(), widths, activations, True)


@gpu
@pytest.mark.parametrize("n,B", [(0, 5), (2, 0)])
def test_empty_launch(n, B):
    import evotorch_amd._C as C

    out = C.population_mlp_forward_shared_bf16(torch.ones(n, L).cuda(), torch.ones(B, 6).cuda(), W, A, True)
    assert out.shape == (n, B, 3)


def test_cpu_chain_rounds_weights_x_and_hidden_only():
    """Pins the semantics without a device: one rounding of W, x and the hidden layer, nothing else."""
    widths, activations, has_bias = STACKS["odd_tanh"]
    params, x = _inputs(widths, has_bias, 4, 9)
    out = ops.population_forward_shared_bf16(params, x, widths, activations, has_bias)

    def rounded(t):
        return t.bfloat16().float()

    W0, b0, W1, b1 = params[:, :85].reshape(4, 17, 5), params[:, 85:102], params[:, 102:153].reshape(4, 3, 17), params[:, 153:]
    hidden = torch.tanh(torch.einsum("bk,njk->nbj", rounded(x), rounded(W0)) + b0[:, None])
    expected = torch.einsum("nbk,njk->nbj", rounded(hidden), rounded(W1)) + b1[:, None]
    assert out.shape == (4, 9, 3) and torch.allclose(out, expected)
