"""Functional-ized modules: run an nn.Module from a flat parameter vector,
and over a whole POPULATION of parameter vectors at once.

Reference parity: /root/reference/src/evotorch/neuroevolution/net/
functional.py (ModuleExpectingFlatParameters :46, make_functional_module
:203) and the vmapped population forward of net/vecrl.py:1261-1265.

MI355X note: the population-batched forward of a dense stack (nn.Linear
layers with Tanh / ReLU between them) is a GEMV chain per member and runs
as ONE kernel launch, `ops.population_forward` (K13,
ops/hip/policy_forward.hip), and the same stack applied by every member to
one shared minibatch (`forward_shared`, SupervisedNE's evaluation) is a
GEMM chain per member on fp32 MFMA, `ops.population_forward_shared` (K14,
ops/hip/policy_forward_shared.hip), or on request on bf16 MFMA,
`ops.population_forward_shared_bf16` (K15,
ops/hip/policy_forward_shared_bf16.hip); `loss_shared` reduces either to
each member's mean MSE or cross-entropy in the same launch,
`ops.population_loss_shared` (K17, ops/hip/policy_loss.h). A `MultiLayered` stack with one
`RNN` or `LSTM` layer is recognised too (`recurrent_stack_description`);
`models.Policy` runs its step as one launch,
`ops.population_forward_recurrent` (K16,
ops/hip/policy_forward_recurrent.hip), when asked to. Every other module goes through
`torch.func.vmap` over `functional_call`, which lowers population-batched
layers to library calls. The whole-episode fused path for the synthetic
environment lives in evotorch_amd/ops/hip/rollout.hip.
"""

import copy
from typing import Optional, Tuple

import torch
from torch import nn

from .. import ops
from .layers import LSTM, RNN
from .multilayered import MultiLayered

__all__ = [
    "ModuleExpectingFlatParameters",
    "dense_stack_description",
    "make_functional_module",
    "recurrent_stack_description",
]


def dense_stack_description(net: nn.Module) -> Optional[Tuple[list, list, bool]]:
    """(widths, activation codes, has_bias) when `net` is a dense stack that
    `ops.population_forward` computes, else None.

    A dense stack is exactly an `nn.Linear`, or an `nn.Sequential` /
    `MultiLayered` whose children are exactly `nn.Linear`, `nn.Tanh` and
    `nn.ReLU` instances (subclasses may override forward and are not
    recognised): 1 to 4 Linear layers that chain, widths up to 1024, all
    with a bias or none, at most one activation after each Linear and none
    before the first, no buffers, no module used twice."""
    if type(net) is nn.Linear:
        layers = [net]
    elif type(net) in (nn.Sequential, MultiLayered):
        layers = list(net)
    else:
        return None
    if len(set(map(id, layers))) != len(layers) or next(net.buffers(), None) is not None:
        return None
    codes = {nn.Tanh: ops.POPULATION_FORWARD_ACTIVATIONS.index("tanh"), nn.ReLU: ops.POPULATION_FORWARD_ACTIVATIONS.index("relu")}
    widths, activations, biases = [], [], []
    after_linear = False
    for layer in layers:
        if type(layer) is nn.Linear:
            if widths and widths[-1] != layer.in_features:
                return None
            if not widths:
                widths.append(layer.in_features)
            widths.append(layer.out_features)
            activations.append(ops.POPULATION_FORWARD_ACTIVATIONS.index("identity"))
            biases.append(layer.bias is not None)
            after_linear = True
        elif type(layer) in codes and after_linear:
            activations[-1] = codes[type(layer)]
            after_linear = False
        else:
            return None
    if not 1 <= len(activations) <= ops.POPULATION_FORWARD_MAX_LAYERS or len(set(biases)) != 1:
        return None
    if not all(1 <= w <= ops.POPULATION_FORWARD_MAX_WIDTH for w in widths):
        return None
    return widths, activations, biases[0]


def recurrent_stack_description(net: nn.Module) -> Optional[Tuple[list, list, list, bool, int]]:
    """(kinds, widths, activation codes, has_bias, state_index) when `net`
    is a recurrent stack that `ops.population_forward_recurrent` computes,
    else None.

    A recurrent stack is exactly a `MultiLayered` (what `>>` builds) whose
    children are exactly `nn.Linear`, `nn.Tanh`, `nn.ReLU`, `layers.RNN` and
    `layers.LSTM` instances (no subclasses), with exactly one recurrent
    child; `state_index` is that child's position, its key in the state
    dict. Otherwise the rules are `dense_stack_description`'s: 1 to 4
    weighted layers that chain, widths up to 1024, the Linear layers all
    with a bias or none, at most one activation after each Linear (none
    after the recurrent layer, whose output is its state), no buffers, no
    module used twice. `has_bias` is True for a stack without a Linear."""
    if type(net) is not MultiLayered:
        return None
    layers = list(net)
    if len(set(map(id, layers))) != len(layers) or next(net.buffers(), None) is not None:
        return None
    names = ops.POPULATION_FORWARD_ACTIVATIONS
    codes = {nn.Tanh: names.index("tanh"), nn.ReLU: names.index("relu")}
    kinds, widths, activations, biases, state_index = [], [], [], [], None
    after_linear = False
    for index, layer in enumerate(layers):
        if type(layer) in codes:
            if not after_linear:
                return None
            activations[-1] = codes[type(layer)]
            after_linear = False
            continue
        if type(layer) is nn.Linear:
            kind, k, j, act = "dense", layer.in_features, layer.out_features, "identity"
            biases.append(layer.bias is not None)
        elif type(layer) is RNN and state_index is None:
            kind, k, j = "rnn", layer.input_size, layer.hidden_size
            act = "tanh" if layer._act is torch.tanh else "relu"
        elif type(layer) is LSTM and state_index is None:
            kind, k, j, act = "lstm", layer.input_size, layer.hidden_size, "identity"
        else:
            return None
        if widths and widths[-1] != k:
            return None
        if kind != "dense":
            state_index = index
        widths += [j] if widths else [k, j]
        kinds.append(ops.POPULATION_FORWARD_KINDS.index(kind))
        activations.append(names.index(act))
        after_linear = kind == "dense"
    if state_index is None or len(kinds) > ops.POPULATION_FORWARD_MAX_LAYERS or len(set(biases)) > 1:
        return None
    if not all(1 <= w <= ops.POPULATION_FORWARD_MAX_WIDTH for w in widths):
        return None
    return kinds, widths, activations, (biases[0] if biases else True), state_index


class ModuleExpectingFlatParameters:
    """Wraps an nn.Module as a pure function `f(flat_params, *inputs)`.

    With a 2-D `flat_params` (popsize × L) the call is vmapped across the
    population: `f(params_2d, batched_inputs)` evaluates every member's
    network in one batched pass. Dense stacks (`dense_stack_description`)
    with fp32 ROCm parameters run that pass as one HIP kernel launch.
    """

    def __init__(self, net: nn.Module, *, disable_autograd_tracking: bool = True):
        self._net = copy.deepcopy(net)
        self._param_shapes = [(name, p.shape, p.numel()) for name, p in self._net.named_parameters()]
        self._length = sum(n for _, _, n in self._param_shapes)
        self._buffers = dict(self._net.named_buffers())
        self._dense_stack = dense_stack_description(self._net)
        self._recurrent_stack = recurrent_stack_description(self._net)  # K16's, taken by models.Policy on request
        self._shared_tile = None  # K14's batch tile for this stack, asked of the extension once
        self._loss_tile = None  # K17's, for the fp32 loss layout
        if disable_autograd_tracking:
            for p in self._net.parameters():
                p.requires_grad_(False)

    @property
    def parameter_count(self) -> int:
        return self._length

    def parameter_dict(self, flat: torch.Tensor) -> dict:
        out = {}
        offset = 0
        for name, shape, numel in self._param_shapes:
            out[name] = flat[offset : offset + numel].reshape(shape)
            offset += numel
        return out

    def _single(self, flat: torch.Tensor, *inputs):
        params = self.parameter_dict(flat)
        return torch.func.functional_call(self._net, {**params, **self._buffers}, inputs)

    def _takes_kernel(self, flat_params: torch.Tensor, inputs: tuple) -> bool:
        """Whether this 2-D call is `ops.population_forward`'s: a dense
        stack, fp32 ROCm parameters, one fp32 (n, D0) input beside them, no
        gradient asked for, and the HIP path switched on."""
        if self._dense_stack is None or len(inputs) != 1 or not isinstance(inputs[0], torch.Tensor):
            return False
        x = inputs[0]
        if flat_params.device.type != "cuda" or flat_params.dtype != torch.float32:
            return False
        if x.device != flat_params.device or x.dtype != torch.float32:
            return False
        if x.shape != (flat_params.shape[0], self._dense_stack[0][0]) or flat_params.shape[1] != self._length:
            return False
        if torch.is_grad_enabled() and (flat_params.requires_grad or x.requires_grad):
            return False  # the kernel has no backward
        return ops.hip_for(flat_params) is not None

    def takes_shared_kernel(self, flat_params: torch.Tensor, x, precision: str = "fp32") -> bool:
        """Whether `forward_shared(flat_params, x, precision)` is one kernel
        launch: a dense stack, 2-D fp32 ROCm parameters, `x` 2-D fp32 of
        width D0 on the same device, no gradient asked for, the HIP path
        switched on, and, for "fp32" (`ops.population_forward_shared`),
        widths narrow enough for that kernel's 32-row batch tiles (wider
        stacks measured slower than the vmap path). "bf16"
        (`ops.population_forward_shared_bf16`) takes stacks of any width."""
        if precision not in ("fp32", "bf16"):
            raise ValueError(f'precision must be "fp32" or "bf16", got {precision!r}')
        if self._dense_stack is None or not isinstance(x, torch.Tensor):
            return False
        if flat_params.device.type != "cuda" or flat_params.dtype != torch.float32:
            return False
        if x.device != flat_params.device or x.dtype != torch.float32:
            return False
        if flat_params.ndim != 2 or flat_params.shape[1] != self._length:
            return False
        if x.ndim != 2 or x.shape[1] != self._dense_stack[0][0]:
            return False
        if torch.is_grad_enabled() and (flat_params.requires_grad or x.requires_grad):
            return False  # the kernels have no backward
        mod = ops.hip_for(flat_params)
        if mod is None:
            return False
        if precision == "bf16":
            return True
        if self._shared_tile is None:
            self._shared_tile = mod.population_mlp_forward_shared_batch_tile(self._dense_stack[0])
        return self._shared_tile >= ops.POPULATION_FORWARD_SHARED_MIN_TILE

    def forward_shared(self, flat_params: torch.Tensor, x: torch.Tensor, precision: str = "fp32") -> torch.Tensor:
        """Every member of the 2-D `flat_params` (n, L) applied to the same
        input batch `x`: (n, B, *out). One `ops.population_forward_shared`
        launch where `takes_shared_kernel` holds, else vmapped.

        `precision="bf16"` asks for `ops.population_forward_shared_bf16`
        instead: weights, `x` and hidden activations rounded to bfloat16,
        sums, bias and activations in fp32. Where `takes_shared_kernel`
        does not hold for it, the call is the vmapped fp32 one."""
        if self.takes_shared_kernel(flat_params, x, precision):
            if precision == "bf16":
                return ops.population_forward_shared_bf16(flat_params, x, *self._dense_stack)
            return ops.population_forward_shared(flat_params, x, *self._dense_stack)
        return torch.func.vmap(self._single, in_dims=(0, None))(flat_params, x)

    def takes_loss_kernel(self, flat_params: torch.Tensor, x, y, loss: str, precision: str = "fp32") -> bool:
        """Whether `loss_shared(flat_params, x, y, loss, precision)` is one
        launch of `ops.population_loss_shared`'s kernel: everything
        `takes_shared_kernel` asks (for "fp32" the tile rule is asked of
        the loss layout, whose rows also hold the last layer's output), and
        a `y` the kernel reads as it is: fp32 of shape exactly
        (B, D_last) for "mse" (no broadcasting case), int64 class indices
        of shape (B,) for "cross_entropy", on the parameters' device."""
        if loss not in ops.POPULATION_LOSS_KINDS:
            raise ValueError(f"loss must be one of {ops.POPULATION_LOSS_KINDS}, got {loss!r}")
        if not self.takes_shared_kernel(flat_params, x, precision) or not isinstance(y, torch.Tensor):
            return False
        if y.device != flat_params.device or y.requires_grad:
            return False
        if loss == "mse":
            if y.dtype != torch.float32 or y.shape != (x.shape[0], self._dense_stack[0][-1]):
                return False
        elif y.dtype != torch.int64 or y.shape != (x.shape[0],):
            return False
        if precision == "bf16":
            return True
        if self._loss_tile is None:
            self._loss_tile = ops.hip_for(flat_params).population_mlp_loss_shared_batch_tile(self._dense_stack[0], False)
        return self._loss_tile >= ops.POPULATION_FORWARD_SHARED_MIN_TILE

    def loss_shared(self, flat_params: torch.Tensor, x: torch.Tensor, y: torch.Tensor, loss: str, precision: str = "fp32") -> torch.Tensor:
        """The mean `loss` ("mse" or "cross_entropy") of every member of
        the 2-D `flat_params` (n, L) on the same minibatch `(x, y)`: (n,).
        One `ops.population_loss_shared` launch for forward and loss
        together where `takes_loss_kernel` holds; else `forward_shared`
        followed by the torch loss per member."""
        if self.takes_loss_kernel(flat_params, x, y, loss, precision):
            return ops.population_loss_shared(flat_params, x, y, *self._dense_stack, loss=loss, precision=precision)
        loss_func = torch.nn.functional.mse_loss if loss == "mse" else torch.nn.functional.cross_entropy
        return torch.func.vmap(lambda p: loss_func(p, y))(self.forward_shared(flat_params, x, precision))

    def __call__(self, flat_params: torch.Tensor, *inputs):
        if flat_params.ndim == 1:
            return self._single(flat_params, *inputs)
        if flat_params.ndim == 2:
            if self._takes_kernel(flat_params, inputs):
                return ops.population_forward(flat_params, inputs[0], *self._dense_stack)
            return torch.func.vmap(self._single)(flat_params, *inputs)
        raise ValueError(f"flat_params must be 1-D or 2-D, got ndim={flat_params.ndim}")


def make_functional_module(net: nn.Module, *, disable_autograd_tracking: bool = True) -> ModuleExpectingFlatParameters:
    return ModuleExpectingFlatParameters(net, disable_autograd_tracking=disable_autograd_tracking)
