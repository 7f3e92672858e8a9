"""K16 `ops.population_forward_recurrent` / `_C.population_recurrent_forward`:
one step of a stack with one RNN or LSTM layer for every member in one launch
(ops/hip/policy_forward_recurrent.hip).

Numerics are held against the op's eager chain in float64; the bound is the
vmap path's own error on the same inputs (see `test_numerics`)."""

import math

import pytest
import torch
from torch import nn

from evotorch_amd import ops
from evotorch_amd.models import MultiLayered, Policy, str_to_net
from evotorch_amd.models.functional import make_functional_module, recurrent_stack_description

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


def gpu(test):
    return pytest.mark.gpu(requires_gpu(test))


# the smallest shapes at which the kernel takes another path
STACKS = {
    "rnn_tails_only": "RNN(3, 2)",  # both segments tail-only, every row misaligned
    "rnn_between_dense": "Linear(5, 17) >> Tanh() >> RNN(17, 9, 'relu') >> Linear(9, 3)",  # units % units per pass != 0
    "lstm_h5": "LSTM(6, 5) >> Linear(5, 2)",  # H % 4 != 0 in the four-gate path
    "lstm_h65": "LSTM(33, 65) >> Linear(65, 1)",  # ragged tail after full words, H past a wave
    "four_layers": "Linear(376, 64) >> Tanh() >> LSTM(64, 64) >> Linear(64, 17)",
    "rnn_g64": "RNN(1024, 8) >> Linear(8, 2)",
    "rnn_h1024": "RNN(8, 1024) >> Linear(1024, 2)",  # the width limit on H
}


def _stack(stack):
    net = str_to_net(STACKS[stack])
    net = net if isinstance(net, MultiLayered) else MultiLayered(net)
    return net, recurrent_stack_description(net)


def _inputs(net, n, seed=0):
    """(params, three observations, h, c | None): every parameter uniform in ±1/sqrt(its fan-in) (biases: their
    layer's), observations and state in ±1."""
    g = torch.Generator().manual_seed(seed)
    parts, fan_in = [], 1
    for p in net.parameters():
        fan_in = p.shape[1] if p.ndim == 2 else fan_in
        parts.append((torch.rand(n, p.numel(), generator=g) * 2 - 1) / math.sqrt(fan_in))
    desc = recurrent_stack_description(net)
    H = desc[1][[k != 0 for k in desc[0]].index(True) + 1]
    obs, h, c = (torch.rand(n, w, generator=g) * 2 - 1 for w in (3 * desc[1][0], H, H))
    return torch.cat(parts, dim=1), obs.reshape(n, 3, -1).unbind(1), h, (c if desc[0].count(2) else None)


def _flat(state):
    (value,) = state.values()
    return list(value) if isinstance(value, tuple) else [value]


@gpu
@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("stack", list(STACKS))
def test_numerics(stack, n):
    """Three chained steps from no state. Over out, h and c of every step: max|kernel - float64| <=
    4 * e_ref + 1e-7, e_ref = max|vmap path - float64| on the GPU (both round the same products and
    differ in summation order only). e_ref <= 1e-4 keeps a bad reference from excusing a bad kernel."""
    net, desc = _stack(stack)
    params, steps, _, _ = _inputs(net, n)
    policy = Policy(net)
    policy.set_parameters(params.cuda())
    exact_state, state, e_ref, e_kernel = (None, None), (None, None), 0.0, 0.0
    for obs in steps:
        exact = ops.population_forward_recurrent(params.double(), obs.double(), *exact_state, *desc[:4])
        got = ops.population_forward_recurrent(params.cuda(), obs.cuda(), *state, *desc[:4])
        with ops.eager_on_gpu():
            vmapped = [policy(obs.cuda())] + _flat(policy.h)
        exact_state, state = exact[1:], got[1:]
        for want, ours, ref in zip(exact, got, vmapped):
            if want is not None:
                assert ours.shape == want.shape and ours.dtype == torch.float32
                e_kernel = max(e_kernel, (ours.cpu().double() - want).abs().max().item())
                e_ref = max(e_ref, (ref.cpu().double() - want).abs().max().item())
    print(f"{stack} n={n}: e_ref={e_ref:.3e} e_kernel={e_kernel:.3e}")
    assert e_ref <= 1e-4
    assert e_kernel <= 4 * e_ref + 1e-7


@gpu
@pytest.mark.parametrize("stack", ["lstm_h5", "four_layers"])
def test_member_is_independent_of_the_population(stack):
    net, desc = _stack(stack)
    params, steps, h, c = _inputs(net, 9, seed=1)
    params, obs, h, c = params.cuda(), steps[0].cuda(), h.cuda(), c.cuda()
    whole = ops.population_forward_recurrent(params, obs, h, c, *desc[:4])
    for rows in ([0], [3], [8], [0, 3, 8]):
        part = ops.population_forward_recurrent(params[rows], obs[rows], h[rows], c[rows], *desc[:4])
        for ours, want in zip(part, whole):
            assert torch.equal(ours, want[rows])


@gpu
@pytest.mark.parametrize("stack", ["rnn_between_dense", "lstm_h5"])
def test_recurrent_policy_takes_the_kernel(stack, monkeypatch):
    net, desc = _stack(stack)
    params, steps, _, _ = _inputs(net, 5, seed=2)
    params, steps = params.cuda(), [obs.cuda() for obs in steps]
    policy = Policy(net, recurrent_kernel=True)
    policy.set_parameters(params)
    mask = torch.tensor([True, False, False, True, False]).cuda()
    state = (None, None)
    for t, obs in enumerate(steps):
        if t == 2:
            policy.reset(mask)
            state = tuple(None if s is None else torch.where(mask[:, None], 0.0, s) for s in state)
        want = ops.population_forward_recurrent(params, obs, *state, *desc[:4])
        state = want[1:]
        assert torch.equal(policy(obs), want[0])
        assert list(policy.h) == [desc[4]] and isinstance(policy.h[desc[4]], tuple) == (state[1] is not None)
        assert all(torch.equal(a, b) for a, b in zip(_flat(policy.h), state))
    # 1-D parameters never reach the kernel
    monkeypatch.setattr(ops, "population_forward_recurrent", None)  # a call would raise
    policy.set_parameters(params[0])
    assert policy(steps[0][0]).shape == (desc[1][-1],)


RNN_K, RNN_W, LSTM_K, LSTM_W = [1, 0], [6, 4, 3], [2, 0], [6, 4, 3]
RNN_L, LSTM_L = 4 * 6 + 4 * 4 + 8 + 15, 4 * (4 * 6 + 4 * 4 + 8) + 15
# name -> (what the error names, params, obs, h, c, kinds, widths, activations); operands are built on the host here
REJECTED = {
    "params_host": ("params", lambda: torch.ones(2, RNN_L), (2, 6), None, None, RNN_K, RNN_W, [1, 0]),
    "params_fp64": ("params", lambda: torch.ones(2, RNN_L, dtype=torch.float64).cuda(), (2, 6), None, None, RNN_K, RNN_W, [1, 0]),
    "L_short": (f"{RNN_L} values per member.*{RNN_L - 1}", lambda: torch.ones(2, RNN_L - 1).cuda(), (2, 6), None, None, RNN_K, RNN_W, [1, 0]),
    "obs_width": ("obs", lambda: torch.ones(2, RNN_L).cuda(), (2, 7), None, None, RNN_K, RNN_W, [1, 0]),
    "h_shape": ("h must be", lambda: torch.ones(2, RNN_L).cuda(), (2, 6), (4, 2), None, RNN_K, RNN_W, [1, 0]),
    "c_missing": ("c must be", lambda: torch.ones(2, LSTM_L).cuda(), (2, 6), (2, 4), None, LSTM_K, LSTM_W, [0, 0]),
    "two_recurrent": ("kinds", lambda: torch.ones(2, 99).cuda(), (2, 6), None, None, [1, 1], RNN_W, [1, 1]),
    "H_1025": ("widths", lambda: torch.ones(2, 99).cuda(), (2, 6), None, None, [1], [6, 1025], [1]),
}


@gpu
@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_operand(case):
    import evotorch_amd._C as C

    names, params, obs, h, c, kinds, widths, activations = REJECTED[case]
    h, c = (None if shape is None else torch.ones(shape).cuda() for shape in (h, c))
    with pytest.raises(RuntimeError, match=names):
        C.population_recurrent_forward(params(), torch.ones(obs).cuda(), h, c, kinds, widths, activations, True)


@gpu
def test_empty_population():
    import evotorch_amd._C as C

    out, h, c = C.population_recurrent_forward(torch.ones(0, LSTM_L).cuda(), torch.ones(0, 6).cuda(), None, None,
                                               LSTM_K, LSTM_W, [0, 0], True)
    assert out.shape == (0, 3) and h.shape == (0, 4) and c.shape == (0, 4)


@pytest.mark.parametrize("stack", ["rnn_between_dense", "lstm_h5"])
def test_cpu_chain_is_the_module(stack):
    """Pins the parameter layout and the gate order where they can be checked without a device."""
    net, desc = _stack(stack)
    params, steps, _, _ = _inputs(net, 6)
    fmodule, state, vstate = make_functional_module(net), (None, None), None
    for obs in steps[:2]:
        out, *state = ops.population_forward_recurrent(params, obs, *state, *desc[:4])
        vout, vstate = torch.func.vmap(fmodule._single)(params, obs, *([] if vstate is None else [vstate]))
        for ours, want in zip([out] + [s for s in state if s is not None], [vout] + _flat(vstate)):
            torch.testing.assert_close(ours, want)


def test_unrecognised_nets():
    assert recurrent_stack_description(nn.Sequential(nn.Linear(3, 2))) is None
    assert recurrent_stack_description(str_to_net("RNN(3, 2) >> Clip(-1.0, 1.0)")) is None
    assert recurrent_stack_description(str_to_net("RNN(3, 2) >> LSTM(2, 2)")) is None
    assert make_functional_module(str_to_net("RNN(3, 2) >> Linear(2, 1)"))._dense_stack is None


@gpu
def test_vecenvne_recurrent_kernel_graph_matches_eager():
    """The comparison of tests/test_gpu_e2e.py's test_vecenvne_hip_graph_matches_eager, on the K16 policy."""
    from evotorch_amd.algorithms import PGPE
    from evotorch_amd.neuroevolution import SyntheticTorchEnv, VecEnvNE

    def env_factory(num_envs):
        return SyntheticTorchEnv(num_envs=num_envs, episode_length=12, obs_dim=32, act_dim=8, rank=8, device="cuda:0")

    def run(use_graph):
        prob = VecEnvNE(env_factory, "RNN(obs_length, 16) >> Linear(16, act_length)", device="cuda:0", seed=7,
                        use_hip_graph=use_graph, recurrent_policy_kernel=True, observation_normalization=False)
        searcher = PGPE(prob, popsize=6, center_learning_rate=0.05, stdev_learning_rate=0.1,
                        stdev_init=0.1, distributed=True)
        searcher.run(4)
        (h,) = prob._policy.h.values()
        assert list(prob._policy.h) == [0] and h.shape == (6, 16)
        return searcher.status["mean_eval"], searcher._distribution.mu.clone(), prob.interaction_count

    eval_e, mu_e, steps_e = run(False)
    eval_g, mu_g, steps_g = run(True)
    assert steps_e == steps_g
    torch.testing.assert_close(mu_g, mu_e, rtol=1e-4, atol=1e-5)
    assert abs(float(eval_g) - float(eval_e)) < 1e-2 * max(1.0, abs(float(eval_e)))
