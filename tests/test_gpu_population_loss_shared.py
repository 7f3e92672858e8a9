"""K17 `ops.population_loss_shared` / `_C.population_mlp_loss_shared`: the
shared-minibatch forward (K14 on fp32 MFMA, K15 on bf16 MFMA) with the mean MSE
or cross-entropy fused into its last epilogue (ops/hip/policy_loss.h), and its
routing from `SupervisedNE`.

The criterion is K13/K14/K16's: `e_kernel <= 4 * e_ref + 1e-7` against a float64
oracle, `e_ref` being the error of the unfused fp32 path on the same inputs."""

import pytest
import torch
from torch import nn
from torch.nn import functional as F

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
    "k3_identity": ([3, 2], [ID], True),
    "odd_tanh": ([5, 17, 3], [TANH, ID], True),
    "one_column": ([33, 64, 65, 1], [RELU, TANH, ID], True),  # D_last = 1, the narrowest row
    "no_bias": ([20, 9, 4], [TANH, RELU], False),
    "wide_row": ([8, 70], [ID], True),  # 70 columns: 64 lanes a row, one lane pass past 64
    "widest_lds": ([16, 1024, 16], [TANH, ID], True),  # smallest fp32 tile
    "widest_row": ([16, 1024, 1024], [TANH, ID], True),  # 16 passes a lane; the bf16 layout only fits 16-row tiles
}
SIZES = [(1, 1), (3, 17), (5, 130)]  # 130 rows: several tiles and a ragged last one for every tile size
LOSSES = {"mse": F.mse_loss, "cross_entropy": F.cross_entropy}


def _inputs(stack, n, B, loss, seed=0):
    """params (n, L), x (B, D0), y for `loss`, and the stack as a functional nn module (the vmap path)."""
    widths, activations, has_bias = STACKS[stack]
    g = torch.Generator().manual_seed(seed)
    L = sum(j * k + (j if has_bias else 0) for k, j in zip(widths[:-1], widths[1:]))
    params, x = 0.3 * torch.randn(n, L, generator=g), torch.randn(B, widths[0], generator=g)
    y = torch.randn(B, widths[-1], generator=g) if loss == "mse" else torch.randint(0, widths[-1], (B,), generator=g)
    layers = []
    for k, j, act in zip(widths[:-1], widths[1:], activations):
        layers += [nn.Linear(k, j, bias=has_bias)] + [[], [nn.Tanh()], [nn.ReLU()]][act]
    return params, x, y, make_functional_module(nn.Sequential(*layers))


def _check(what, kernel, reference, exact):
    e_ref = (reference.double().cpu() - exact.cpu()).abs().max().item()
    e_kernel = (kernel.double().cpu() - exact.cpu()).abs().max().item()
    print(f"{what}: e_ref={e_ref:.3e} e_kernel={e_kernel:.3e}")
    assert kernel.dtype == torch.float32 and kernel.shape == exact.shape
    assert e_kernel <= 4 * e_ref + 1e-7


def _unfused(fmodule, params, x, y, loss):
    """Today's path on the GPU: the vmap forward, then the torch loss per member."""
    with ops.eager_on_gpu():
        preds = fmodule.forward_shared(params.cuda(), x.cuda())
    return torch.func.vmap(lambda p: LOSSES[loss](p, y.cuda()))(preds)


@gpu
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("n,B", SIZES)
@pytest.mark.parametrize("stack", list(STACKS))
def test_numerics_fp32(stack, n, B, loss):
    params, x, y, fmodule = _inputs(stack, n, B, loss)
    exact = ops.population_loss_shared(params.double(), x.double(), y, *STACKS[stack], loss=loss)
    out = ops.population_loss_shared(params.cuda(), x.cuda(), y.cuda(), *STACKS[stack], loss=loss)
    _check(f"{stack} n={n} B={B} {loss}", out, _unfused(fmodule, params, x, y, loss), exact)


@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("n,B", SIZES)
@pytest.mark.parametrize("stack", list(STACKS))
def test_loss_phase_on_the_unfused_kernels_output(stack, n, B, loss, precision):
    params, x, y, _ = (t.cuda() if isinstance(t, torch.Tensor) else t for t in _inputs(stack, n, B, loss))
    forward = ops.population_forward_shared_bf16 if precision == "bf16" else ops.population_forward_shared
    preds = forward(params, x, *STACKS[stack])
    exact = torch.stack([LOSSES[loss](p.double(), y.double() if loss == "mse" else y) for p in preds])
    reference = torch.stack([LOSSES[loss](p, y) for p in preds])
    out = ops.population_loss_shared(params, x, y, *STACKS[stack], loss=loss, precision=precision)
    _check(f"{stack} n={n} B={B} {loss} {precision}", out, reference, exact)


@gpu
@pytest.mark.parametrize("case", ["some_ignored", "all_ignored", "logits_80"])
def test_cross_entropy_edges(case):
    params, x, y, fmodule = _inputs("odd_tanh", 3, 17, "cross_entropy")
    if case == "some_ignored":
        y[[0, 5, 16]] = -100
    elif case == "all_ignored":
        y[:] = -100
    else:  # the last layer (17 x 3 weights and 3 biases) scaled until the logits reach about +-80
        params[:, 5 * 17 + 17 :] *= 50
        logits = ops.population_forward_shared(params.double(), x.double(), *STACKS["odd_tanh"])
        assert 60 < logits.abs().max() < 100
    exact = ops.population_loss_shared(params.double(), x.double(), y, *STACKS["odd_tanh"], loss="cross_entropy")
    reference = _unfused(fmodule, params, x, y, "cross_entropy")
    for precision in ("fp32", "bf16"):
        out = ops.population_loss_shared(params.cuda(), x.cuda(), y.cuda(), *STACKS["odd_tanh"], loss="cross_entropy", precision=precision)
        if case == "all_ignored":
            assert exact.isnan().all() and reference.isnan().all() and out.isnan().all()
        elif precision == "fp32":
            assert exact.isfinite().all() and out.isfinite().all()
            _check(case, out, reference, exact)
        else:
            assert out.isfinite().all()
    outside = y.clone()
    outside[3] = 3  # one past the last class: NaN for every member, and no read outside the tile
    out = ops.population_loss_shared(params.cuda(), x.cuda(), outside.cuda(), *STACKS["odd_tanh"], loss="cross_entropy")
    assert out.isnan().all()


@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("stack", list(STACKS))
def test_loss_is_independent_of_the_launch(stack, loss, precision):
    params, x, y, _ = (t.cuda() if isinstance(t, torch.Tensor) else t for t in _inputs(stack, 5, 130, loss, seed=1))
    whole = ops.population_loss_shared(params, x, y, *STACKS[stack], loss=loss, precision=precision)
    alone = ops.population_loss_shared(params[2:3], x, y, *STACKS[stack], loss=loss, precision=precision)
    assert torch.equal(whole[2:3], alone)
    assert torch.equal(whole, ops.population_loss_shared(params, x, y, *STACKS[stack], loss=loss, precision=precision))


class _OwnLoss(SupervisedNE):
    def _loss(self, y_hat, y):
        return F.mse_loss(y_hat, y)


@gpu
@pytest.mark.parametrize("loss", list(LOSSES))
def test_supervisedne_takes_the_fused_loss(loss, monkeypatch):
    g = torch.Generator().manual_seed(4)
    X = torch.randn(96, 8, generator=g)
    Y = torch.randn(96, 3, generator=g) if loss == "mse" else torch.randint(0, 3, (96,), generator=g)
    net = nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 3))
    values = 0.3 * torch.randn(7, 8 * 16 + 16 + 16 * 3 + 3, generator=g)
    recognised = nn.MSELoss() if loss == "mse" else F.cross_entropy
    forwards, real_forward = [], ops.population_forward_shared
    monkeypatch.setattr(ops, "population_forward_shared", lambda *a: forwards.append(1) or real_forward(*a))

    def evaluate(loss_func, Y=Y, cls=SupervisedNE):
        # same seed: the CPU DataLoader generator draws the same minibatch
        problem = cls(torch.utils.data.TensorDataset(X, Y), net, loss_func, minibatch_size=32, device="cuda:0", seed=3)
        batch = SolutionBatch(problem, popsize=7)
        batch.access_values()[:] = values.to(batch.device)
        problem.evaluate(batch)
        return problem, torch.Tensor.as_subclass(batch.evals[:, 0], torch.Tensor)

    problem, fused = evaluate(recognised)
    assert forwards == []
    _, unfused = evaluate(lambda y_hat, y: recognised(y_hat, y))
    assert forwards == [1]
    xb, yb = next(iter(problem.make_dataloader()))
    exact = ops.population_loss_shared(values.double(), xb.double(), yb, [8, 16, 3], [TANH, ID], True, loss=loss)
    _check(f"fitness {loss}", fused, unfused, exact)

    # not routed: an overridden _loss, and a (B,) target for a (B, 1) output (mse_loss broadcasts it)
    monkeypatch.setattr(ops, "population_loss_shared", None)  # a call would raise
    evaluate(nn.MSELoss(), Y=torch.randn(96, 3, generator=g), cls=_OwnLoss)
    net = nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 1))
    values = values[:, : 8 * 16 + 16 + 16 + 1]
    with pytest.warns(UserWarning, match="broadcasting"):
        evaluate(nn.MSELoss(), Y=torch.randn(96, generator=g))
    assert len(forwards) == 3


W, A = [6, 4, 3], [TANH, ID]
L = 6 * 4 + 4 + 4 * 3 + 3
# name -> (what the error names, y, loss_kind); None: accepted
OPERANDS = {
    "mse": (None, lambda: torch.ones(5, 3).cuda(), 0),
    "cross_entropy": (None, lambda: torch.ones(5, dtype=torch.int64).cuda(), 1),
    "mse_y_int64": ("y must be Float", lambda: torch.ones(5, 3, dtype=torch.int64).cuda(), 0),
    "ce_y_int32": ("y must be Long", lambda: torch.ones(5, dtype=torch.int32).cuda(), 1),
    "mse_y_short": ("y must have 15 elements", lambda: torch.ones(5, 2).cuda(), 0),
    "ce_y_long": ("y must have 5 elements", lambda: torch.ones(6, dtype=torch.int64).cuda(), 1),
    "y_host": ("y must be on cuda", lambda: torch.ones(5, 3), 0),
    "y_strided": ("y must be contiguous", lambda: torch.ones(5, 6).cuda()[:, ::2], 0),
    "loss_kind_2": ("loss_kind must be 0", lambda: torch.ones(5, 3).cuda(), 2),
}


@gpu
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", list(OPERANDS))
def test_operands(case, bf16):
    import evotorch_amd._C as C

    names, y, loss_kind = OPERANDS[case]
    params, x = torch.ones(2, L).cuda(), torch.ones(5, 6).cuda()
    if names is None:
        assert C.population_mlp_loss_shared(params, x, y(), W, A, True, loss_kind, bf16).shape == (2,)
        assert C.population_mlp_loss_shared(params[:0], x, y(), W, A, True, loss_kind, bf16).shape == (0,)
        assert C.population_mlp_loss_shared(params, x[:0], y()[:0], W, A, True, loss_kind, bf16).isnan().all()
    else:
        with pytest.raises(RuntimeError, match=names):
            C.population_mlp_loss_shared(params, x, y(), W, A, True, loss_kind, bf16)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("loss", list(LOSSES))
def test_cpu_chain_is_the_torch_loss_per_member(loss, precision):
    params, x, y, _ = _inputs("odd_tanh", 4, 9, loss)
    forward = ops.population_forward_shared_bf16 if precision == "bf16" else ops.population_forward_shared
    preds = forward(params.double(), x.double(), *STACKS["odd_tanh"])
    expected = torch.stack([LOSSES[loss](p, y.double() if loss == "mse" else y) for p in preds])
    out = ops.population_loss_shared(params.double(), x.double(), y, *STACKS["odd_tanh"], loss=loss, precision=precision)
    assert out.shape == (4,) and torch.equal(out, expected)
    with pytest.raises(ValueError, match="expected y"):
        ops.population_loss_shared(params, x, y[:-1], *STACKS["odd_tanh"], loss=loss)
    with pytest.raises(ValueError, match="loss must be"):
        ops.population_loss_shared(params, x, y, *STACKS["odd_tanh"], loss="l1")
