"""Policy: a functional-ized network evaluated over a whole population,
with auto-managed (and maskable-reset) recurrent state.

Reference parity: the `Policy` class of
/root/reference/src/evotorch/neuroevolution/net/vecrl.py:1019-1315
(vmapped call :1261-1265, masked state reset via reset_tensors :866).

The parameters tensor may be 1-D (single member) or 2-D (population);
2-D parameters run the whole population per step as a batched forward:
one `ops.population_forward` launch (K13) for Linear/Tanh/ReLU stacks on a
ROCm device, the vmapped `functional_call` for every other module. With
`recurrent_kernel=True` a `MultiLayered` stack holding one RNN or LSTM
layer takes one `ops.population_forward_recurrent` launch (K16) per step.
"""

from typing import Any, Optional, Union

import torch
from torch import nn

from .. import ops
from .functional import make_functional_module
from .parser import str_to_net

__all__ = ["Policy", "reset_tensors"]


def reset_tensors(container: Any, mask: torch.Tensor) -> Any:
    """Recursively zero the rows of every tensor in `container` selected by
    the boolean `mask` (reference net/vecrl.py:866)."""
    if isinstance(container, torch.Tensor):
        m = mask
        while m.ndim < container.ndim:
            m = m.unsqueeze(-1)
        return torch.where(m, torch.zeros_like(container), container)
    if isinstance(container, dict):
        return {k: reset_tensors(v, mask) for k, v in container.items()}
    if isinstance(container, (list, tuple)):
        items = [reset_tensors(v, mask) for v in container]
        return type(container)(items) if isinstance(container, list) else tuple(items)
    return container


class Policy:
    def __init__(self, net: Union[str, nn.Module], recurrent_kernel: bool = False, **constants):
        """`recurrent_kernel=True` opts a recognised recurrent stack
        (`functional.recurrent_stack_description`) with 2-D fp32 ROCm
        parameters into `ops.population_forward_recurrent`; its results
        differ from the vmapped path's in summation order only."""
        if isinstance(net, str):
            net = str_to_net(net, **constants)
        self._net = net
        self._fmodule = make_functional_module(net)
        self._recurrent_kernel = bool(recurrent_kernel)
        self._params: Optional[torch.Tensor] = None
        self._state: Optional[Any] = None

    @property
    def parameter_count(self) -> int:
        return self._fmodule.parameter_count

    @property
    def parameters(self) -> Optional[torch.Tensor]:
        return self._params

    @property
    def parameter_length(self) -> int:  # reference vecrl.py alias
        return self.parameter_count

    @property
    def wrapped_module(self) -> nn.Module:
        """The underlying torch module (reference vecrl.py: wrapped_module)."""
        return self.net

    @property
    def net(self) -> nn.Module:
        return self._net

    @property
    def h(self) -> Optional[Any]:
        return self._state

    def set_parameters(self, params: torch.Tensor, *, reset: bool = True):
        if params.shape[-1] != self.parameter_count:
            raise ValueError(f"Expected parameter vectors of length {self.parameter_count}, got {params.shape[-1]}")
        self._params = params
        if reset:
            self._state = None

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        if self._params is None:
            raise RuntimeError("Call set_parameters first")
        if self._recurrent_kernel and self._takes_recurrent_kernel(obs):
            *stack, state_index = self._fmodule._recurrent_stack
            state = None if self._state is None else self._state[state_index]
            h, c = (state, None) if state is None or isinstance(state, torch.Tensor) else state
            out, new_h, new_c = ops.population_forward_recurrent(self._params, obs, h, c, *stack)
            self._state = {state_index: new_h if new_c is None else (new_h, new_c)}
            return out
        if self._state is None:
            out = self._fmodule(self._params, obs)
        else:
            out = self._call_with_state(obs)
        if isinstance(out, tuple):
            y, self._state = out
            return y
        # probe: maybe the module is stateful but state was None
        return out

    def _takes_recurrent_kernel(self, obs) -> bool:
        """Whether this call is `ops.population_forward_recurrent`'s: a
        recognised recurrent stack, 2-D fp32 ROCm parameters, `obs` fp32
        (n, D0) on that device, no gradient asked for, the HIP path switched
        on, and a state that is None or has the structure that path leaves:
        `{state_index: h}` (RNN) or `{state_index: (h, c)}` (LSTM), fp32
        (n, H) on the device."""
        stack, params = self._fmodule._recurrent_stack, self._params
        if stack is None or not isinstance(obs, torch.Tensor):
            return False
        if params.ndim != 2 or params.device.type != "cuda" or params.dtype != torch.float32:
            return False
        if params.shape[1] != self.parameter_count or obs.shape != (params.shape[0], stack[1][0]):
            return False
        if obs.device != params.device or obs.dtype != torch.float32:
            return False
        kinds, widths, _, _, state_index = stack
        recurrent = next(i for i, kind in enumerate(kinds) if kind != 0)
        parts = []
        if self._state is not None:
            if not isinstance(self._state, dict) or list(self._state) != [state_index]:
                return False
            state = self._state[state_index]
            lstm = ops.POPULATION_FORWARD_KINDS[kinds[recurrent]] == "lstm"
            parts = list(state) if lstm and isinstance(state, tuple) and len(state) == 2 else [state]
            if len(parts) != (2 if lstm else 1):
                return False
            for t in parts:
                if not isinstance(t, torch.Tensor) or t.shape != (params.shape[0], widths[recurrent + 1]):
                    return False
                if t.device != params.device or t.dtype != torch.float32:
                    return False
        if torch.is_grad_enabled() and any(t.requires_grad for t in [params, obs, *parts]):
            return False  # the kernel has no backward
        return ops.hip_for(params) is not None

    def _call_with_state(self, obs: torch.Tensor):
        if self._params.ndim == 2:
            return torch.func.vmap(self._fmodule._single)(self._params, obs, self._state)
        return self._fmodule._single(self._params, obs, self._state)

    def reset(self, mask: Optional[torch.Tensor] = None, *, copy: bool = True):
        """Reset recurrent state: fully (mask=None) or only the rows where
        mask is True (per-env episode restarts)."""
        if mask is None or self._state is None:
            self._state = None
            return
        self._state = reset_tensors(self._state, mask)

    def to_torch_module(self, parameter_vector: torch.Tensor) -> nn.Module:
        """A standalone stateful nn.Module with the given parameters."""
        import copy as _copy

        from .misc import fill_parameters
        from .statefulmodule import ensure_stateful

        net = _copy.deepcopy(self._net)
        fill_parameters(net, torch.as_tensor(parameter_vector))
        return ensure_stateful(net)
