"""K14 `ops.population_forward_shared` / `_C.population_mlp_forward_shared`:
every member's dense stack on one shared minibatch, one launch on fp32 MFMA
(ops/hip/policy_forward_shared.hip), and its routing from
`ModuleExpectingFlatParameters.forward_shared` and `SupervisedNE`.

Numerics are held against the eager chain in float64 on the CPU; the bound is
the vmap path's own error on the same inputs (K13's criterion)."""

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
    "k3_identity": ([3, 2], [ID], True),  # K < 4, N < 16
    "odd_tanh": ([5, 17, 3], [TANH, ID], True),  # N one past a column tile, K tails
    "three_layers": ([33, 64, 65, 1], [RELU, TANH, ID], True),  # K = 65 crosses a super-step by one, N = 1
    "no_bias": ([20, 9, 4], [TANH, RELU], False),
    "longest_k": ([1024, 8], [ID], True),
    "widest_lds": ([16, 1024, 16], [TANH, ID], True),  # widest LDS buffers, smallest batch tile
}
# one row; one past a 16-tile; exactly the largest tile; two 64-tiles plus 2 (uneven for the 16- and 32-row tiles)
SIZES = [(1, 1), (3, 17), (2, 64), (5, 130)]


def _inputs(widths, has_bias, n, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = sum(j * k + (j if has_bias else 0) for k, j in zip(widths[:-1], widths[1:]))
    return 0.3 * torch.randn(n, L, generator=g), torch.randn(B, widths[0], generator=g)


def _module(widths, activations, has_bias):
    layers = []
    for k, j, act in zip(widths[:-1], widths[1:], activations):
        layers.append(nn.Linear(k, j, bias=has_bias))
        layers += [[], [nn.Tanh()], [nn.ReLU()]][act]
    return nn.Sequential(*layers)


@gpu
@pytest.mark.parametrize("n,B", SIZES)
@pytest.mark.parametrize("stack", list(STACKS))
def test_numerics(stack, n, B):
    """max|kernel - float64| <= 4 * e_ref + 1e-7, e_ref = max|vmap path - float64| on the GPU."""
    widths, activations, has_bias = STACKS[stack]
    params, x = _inputs(widths, has_bias, n, B)
    exact = ops.population_forward_shared(params.double(), x.double(), widths, activations, has_bias)
    fmodule = make_functional_module(_module(widths, activations, has_bias))
    with ops.eager_on_gpu():
        vmapped = fmodule.forward_shared(params.cuda(), x.cuda()).cpu()
    out = ops.population_forward_shared(params.cuda(), x.cuda(), widths, activations, has_bias).cpu()
    assert out.shape == (n, B, widths[-1]) and out.dtype == torch.float32
    e_ref = (vmapped.double() - exact).abs().max().item()
    e_kernel = (out.double() - exact).abs().max().item()
    print(f"{stack} n={n} B={B}: e_ref={e_ref:.3e} e_kernel={e_kernel:.3e}")
    assert e_kernel <= 4 * e_ref + 1e-7


@gpu
@pytest.mark.parametrize("stack", list(STACKS))
def test_output_is_independent_of_the_launch(stack):
    widths, activations, has_bias = STACKS[stack]
    params, x = (t.cuda() for t in _inputs(widths, has_bias, 5, 130, seed=1))
    whole = ops.population_forward_shared(params, x, widths, activations, has_bias)
    alone = ops.population_forward_shared(params[2:3], x[70:71], widths, activations, has_bias)
    assert torch.equal(whole[2, 70], alone[0, 0])
    assert torch.equal(whole[:, :17], ops.population_forward_shared(params, x[:17], widths, activations, has_bias))


def _problem(network, X, Y):
    return SupervisedNE(torch.utils.data.TensorDataset(X, Y), network, nn.functional.mse_loss, minibatch_size=32,
                        device="cuda:0", seed=3)


@gpu
def test_supervisedne_takes_the_kernel():
    g = torch.Generator().manual_seed(4)
    X, Y = torch.randn(96, 8, generator=g), torch.randn(96, 1, generator=g)
    net = nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 1))
    values = 0.3 * torch.randn(7, 8 * 16 + 16 + 16 + 1, generator=g)
    evals = []
    for eager in (False, True):
        problem = _problem(net, X, Y)  # same seed: the CPU DataLoader generator draws the same minibatch
        batch = SolutionBatch(problem, popsize=7)
        batch.access_values()[:] = values.to(batch.device)
        if eager:
            with ops.eager_on_gpu():
                problem.evaluate(batch)
        else:
            problem.evaluate(batch)
        evals.append(torch.Tensor.as_subclass(batch.evals[:, 0], torch.Tensor).double().cpu())
    xb, yb = next(iter(_problem(net, X, Y).make_dataloader()))
    preds = ops.population_forward_shared(values.double(), xb.double(), [8, 16, 1], [TANH, ID], True)
    exact = ((preds - yb.double()) ** 2).mean(dim=(1, 2))
    e_kernel, e_ref = ((e - exact).abs().max().item() for e in evals)
    print(f"losses: e_ref={e_ref:.3e} e_kernel={e_kernel:.3e}")
    assert e_kernel <= 4 * e_ref + 1e-7

    fmodule, params, x = problem._fmodule, values.cuda(), xb.cuda()
    assert fmodule.takes_shared_kernel(params, x)
    preds = ops.population_forward_shared(params, x, [8, 16, 1], [TANH, ID], True)
    assert torch.equal(fmodule.forward_shared(params, x), preds)
    # the evaluation itself took the kernel: its losses are the bits of the kernel's predictions
    routed = torch.func.vmap(lambda p: nn.functional.mse_loss(p, yb.cuda()))(preds)
    assert torch.equal(evals[0], routed.double().cpu())


@gpu
@pytest.mark.parametrize("case", ["not_dense", "image_x", "too_wide"])
def test_other_calls_keep_the_vmap_path(case, monkeypatch):
    monkeypatch.setattr(ops, "population_forward_shared", None)  # a call would raise
    g = torch.Generator().manual_seed(5)
    if case == "not_dense":
        from evotorch_amd.models import str_to_net

        fmodule = make_functional_module(str_to_net("Linear(8, 4) >> Clip(-0.5, 0.5)"))
        x = torch.randn(6, 8, generator=g).cuda()
    elif case == "image_x":
        fmodule = make_functional_module(nn.Linear(8, 4))
        x = torch.randn(6, 2, 3, 8, generator=g).cuda()
    else:  # 16-row batch tiles: not routed (ops.POPULATION_FORWARD_SHARED_MIN_TILE)
        fmodule = make_functional_module(nn.Linear(784, 4))
        x = torch.randn(6, 784, generator=g).cuda()
    params = (0.3 * torch.randn(5, fmodule.parameter_count, generator=g)).cuda()
    assert not fmodule.takes_shared_kernel(params, x)
    expected = torch.func.vmap(fmodule._single, in_dims=(0, None))(params, x)
    assert torch.equal(fmodule.forward_shared(params, x), expected)


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
        C.population_mlp_forward_shared(params(), x().cuda(), widths, activations, True)


@gpu
@pytest.mark.parametrize("n,B", [(0, 5), (2, 0)])
def test_empty_launch(n, B):
    import evotorch_amd._C as C

    out = C.population_mlp_forward_shared(torch.ones(n, L).cuda(), torch.ones(B, 6).cuda(), W, A, True)
    assert out.shape == (n, B, 3)


@pytest.mark.parametrize("stack", ["odd_tanh", "no_bias"])
def test_cpu_chain_is_the_module(stack):
    """Pins the parameter layout and the output shape where they can be checked without a device.

    `torch.allclose` at its defaults (rtol 1e-5, atol 1e-8). The chain (einsum) and the module
    (addmm) differ in fp32 summation order by what the CPU's BLAS picks: on the development
    machine max|diff| is 0 (odd_tanh) and 1.2e-7 (no_bias) and both cases pass; on the CPU of
    the MI355X host it is 1.8e-7 for both, and odd_tanh misses the bound on one near-zero
    output, 5.239435e-04 against 5.239733e-04 (3.0e-8 apart, 1.5e-8 allowed)."""
    widths, activations, has_bias = STACKS[stack]
    params, x = _inputs(widths, has_bias, 4, 9)
    fmodule = make_functional_module(_module(widths, activations, has_bias))
    out = ops.population_forward_shared(params, x, widths, activations, has_bias)
    assert out.shape == (4, 9, widths[-1])
    single = torch.stack([fmodule(params[m], x) for m in range(4)])
    excess = (out - single).abs() - (1e-8 + 1e-5 * single.abs())  # what torch.allclose bounds by 0
    worst = excess.argmax()
    print(f"{stack}: max|diff|={(out - single).abs().max().item():.3e}, worst element "
          f"{single.flatten()[worst].item():.6e} vs {out.flatten()[worst].item():.6e}")
    assert torch.allclose(out, single)
    assert torch.allclose(fmodule.forward_shared(params, x), out)
    with pytest.raises(ValueError, match="parameters per member"):
        ops.population_forward_shared(params[:, :-1], x, widths, activations, has_bias)
