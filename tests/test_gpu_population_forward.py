"""K13 `ops.population_forward` / `_C.population_mlp_forward`: the dense
policy stack of every member in one launch (ops/hip/policy_forward.hip).

Numerics are held against the eager chain in float64; the bound is the
vmap path's own error on the same inputs (see `test_numerics`)."""

import math

import pytest
import torch
from torch import nn

from evotorch_amd import ops
from evotorch_amd.models import Policy
from evotorch_amd.models.functional import make_functional_module

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu(test):
    return pytest.mark.gpu(requires_gpu(test))


ID, TANH, RELU = 0, 1, 2

# name -> (widths, activations, has_bias): the smallest shapes at which the kernel takes another path
STACKS = {
    "k3_identity": ([3, 2], [ID], True),  # K below any group width, K % 4 != 0, every row misaligned
    "odd_rows_tanh": ([5, 17, 3], [TANH, ID], True),  # rows no multiple of the rows per pass, odd L
    "three_layers": ([33, 64, 65, 1], [RELU, TANH, ID], True),  # ragged tail after a full word, width past a wave
    "humanoid": ([376, 64, 17], [TANH, ID], True),
    "width_limit": ([1024, 8], [ID], True),
    "no_bias": ([20, 9, 4], [TANH, RELU], False),
}


def _layout_length(widths, has_bias):
    return sum(j * k + (j if has_bias else 0) for k, j in zip(widths[:-1], widths[1:]))


def _inputs(widths, has_bias, n, seed=0):
    """Weights (and biases) uniform in ±1/sqrt(K) per layer, observations in ±1: outputs are O(1)."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k, j in zip(widths[:-1], widths[1:]):
        parts.append((torch.rand(n, j * k + (j if has_bias else 0), generator=g) * 2 - 1) / math.sqrt(k))
    return torch.cat(parts, dim=1), torch.rand(n, widths[0], generator=g) * 2 - 1


def _module(widths, activations, has_bias):
    layers = []
    for k, j, act in zip(widths[:-1], widths[1:], activations):
        layers.append(nn.Linear(k, j, bias=has_bias))
        layers += [[], [nn.Tanh()], [nn.ReLU()]][act]
    return nn.Sequential(*layers)


@gpu
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("stack", list(STACKS))
def test_numerics(stack, n):
    """max|kernel - float64| <= 4 * e_ref + 1e-7, where e_ref = max|vmap path - float64| on the GPU:
    both round the same products and differ in summation order only. e_ref <= 1e-4 keeps a bad
    reference from excusing a bad kernel."""
    widths, activations, has_bias = STACKS[stack]
    params, obs = _inputs(widths, has_bias, n)
    assert params.shape[1] == _layout_length(widths, has_bias)
    exact = ops.population_forward(params.double(), obs.double(), widths, activations, has_bias)
    fmodule = make_functional_module(_module(widths, activations, has_bias))
    with ops.eager_on_gpu():
        vmapped = fmodule(params.cuda(), obs.cuda()).cpu()
    out = ops.population_forward(params.cuda(), obs.cuda(), widths, activations, has_bias).cpu()
    assert out.shape == (n, widths[-1]) and out.dtype == torch.float32
    e_ref = (vmapped.double() - exact).abs().max().item()
    e_kernel = (out.double() - exact).abs().max().item()
    print(f"{stack} n={n}: e_ref={e_ref:.3e} e_kernel={e_kernel:.3e}")
    assert e_ref <= 1e-4
    assert e_kernel <= 4 * e_ref + 1e-7


@gpu
@pytest.mark.parametrize("stack", ["odd_rows_tanh", "humanoid"])
def test_member_is_independent_of_the_population(stack):
    widths, activations, has_bias = STACKS[stack]
    params, obs = (t.cuda() for t in _inputs(widths, has_bias, 37, seed=1))
    whole = ops.population_forward(params, obs, widths, activations, has_bias)
    for i in (0, 3, 36):
        alone = ops.population_forward(params[i : i + 1], obs[i : i + 1], widths, activations, has_bias)
        assert torch.equal(alone[0], whole[i])
        lo, hi = max(i - 1, 0), min(i + 2, 37)
        trio = ops.population_forward(params[lo:hi], obs[lo:hi], widths, activations, has_bias)
        assert torch.equal(trio[i - lo], whole[i])


def _vmap_bits(policy, params, obs):
    return torch.func.vmap(policy._fmodule._single)(params, obs)


@gpu
@pytest.mark.parametrize("as_sequential", [False, True])
def test_dense_policy_takes_the_kernel(as_sequential):
    net = "Linear(obs_length, 16) >> Tanh() >> Linear(16, act_length)"
    policy = Policy(nn.Sequential(nn.Linear(6, 16), nn.Tanh(), nn.Linear(16, 3)) if as_sequential else net,
                    obs_length=6, act_length=3)
    assert policy._fmodule._dense_stack == ([6, 16, 3], [TANH, ID], True)
    params, obs = (t.cuda() for t in _inputs([6, 16, 3], True, 9))
    policy.set_parameters(params)
    assert torch.equal(policy(obs), ops.population_forward(params, obs, [6, 16, 3], [TANH, ID], True))
    with ops.eager_on_gpu():
        assert torch.equal(policy(obs), _vmap_bits(policy, params, obs))
    # 1-D parameters never reach the kernel
    policy.set_parameters(params[0])
    assert torch.equal(policy(obs[0]), policy._fmodule._single(params[0], obs[0]))


@gpu
@pytest.mark.parametrize(
    "net",
    [
        "RNN(obs_length, 8) >> Linear(8, act_length)",
        "Linear(obs_length, 8) >> Tanh() >> Linear(8, act_length) >> Clip(-0.5, 0.5)",
        "Linear(obs_length, 4) >> Linear(4, 4) >> Linear(4, 4) >> Linear(4, 4) >> Linear(4, act_length)",
    ],
)
def test_other_modules_keep_the_vmap_path(net, monkeypatch):
    policy = Policy(net, obs_length=6, act_length=3)
    assert policy._fmodule._dense_stack is None
    monkeypatch.setattr(ops, "population_forward", None)  # a call would raise
    g = torch.Generator().manual_seed(2)
    params = (0.3 * torch.randn(5, policy.parameter_count, generator=g)).cuda()
    obs = torch.randn(5, 6, generator=g).cuda()
    policy.set_parameters(params)
    expected = _vmap_bits(policy, params, obs)
    expected = expected[0] if isinstance(expected, tuple) else expected
    assert torch.equal(policy(obs), expected)


W, A, L = [6, 4, 3], [TANH, ID], _layout_length([6, 4, 3], True)
# name -> (what the error names, params, obs, widths, activations); every operand is built on the host here
REJECTED = {
    "params_host": ("params", lambda: torch.ones(2, L), lambda: torch.ones(2, 6), W, A),
    "params_fp64": ("params", lambda: torch.ones(2, L, dtype=torch.float64).cuda(), lambda: torch.ones(2, 6), W, A),
    "params_strided": ("params", lambda: torch.ones(2, 2 * L).cuda()[:, ::2], lambda: torch.ones(2, 6), W, A),
    "L_short": (f"{L} values per member.*{L - 1}", lambda: torch.ones(2, L - 1).cuda(), lambda: torch.ones(2, 6), W, A),
    "obs_rows": ("obs", lambda: torch.ones(2, L).cuda(), lambda: torch.ones(3, 6), W, A),
    "obs_width": ("obs", lambda: torch.ones(2, L).cuda(), lambda: torch.ones(2, 7), W, A),
    "width_0": ("widths", lambda: torch.ones(2, 6).cuda(), lambda: torch.ones(2, 6), [6, 0, 3], A),
    "width_1025": ("widths", lambda: torch.ones(2, 1025 * 8).cuda(), lambda: torch.ones(2, 1025), [1025, 7], [ID]),
    "five_layers": ("widths", lambda: torch.ones(2, 30).cuda(), lambda: torch.ones(2, 2), [2] * 6, [ID] * 5),
    "activation": ("activations", lambda: torch.ones(2, L).cuda(), lambda: torch.ones(2, 6), W, [TANH, 3]),
}


@gpu
@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_operand(case):
    import evotorch_amd._C as C

    names, params, obs, widths, activations = REJECTED[case]
    with pytest.raises(RuntimeError, match=names):
        C.population_mlp_forward(params(), obs().cuda(), widths, activations, True)


@gpu
def test_accepted_operands_and_empty_population():
    import evotorch_amd._C as C

    params, obs = _inputs(W, True, 2)
    out = C.population_mlp_forward(params.cuda(), obs.cuda(), W, A, True).cpu()
    torch.testing.assert_close(out, ops.population_forward(params, obs, W, A, True))
    empty = C.population_mlp_forward(params[:0].cuda(), obs[:0].cuda(), W, A, True)
    assert empty.shape == (0, 3)


@pytest.mark.parametrize("stack", ["odd_rows_tanh", "no_bias"])
def test_cpu_chain_is_the_module(stack):
    """Pins the parameter layout where it can be checked without a device."""
    widths, activations, has_bias = STACKS[stack]
    params, obs = _inputs(widths, has_bias, 6)
    fmodule = make_functional_module(_module(widths, activations, has_bias))
    assert fmodule._dense_stack == (widths, activations, has_bias)
    torch.testing.assert_close(ops.population_forward(params, obs, widths, activations, has_bias), fmodule(params, obs))
