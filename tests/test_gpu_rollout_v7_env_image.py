"""The v7 rollout kernel's prepacked environment image
(`_C.rollout_env_image_v7`, the `env_image` argument of `_C.rollout_linear`
and `_C.rollout_terminating`).

A launch that is given the image copies the constant range of the kernel's LDS
layout instead of converting it from the fp32 blob, so it must compute the
bits of a launch without it: every comparison here is `torch.equal`.

Inputs are those of tests/test_gpu_rollout_v7_terminating.py: the default
`SyntheticEnvSpec`, its normalization (generator seed 7), SEED = 41,
`params(n) = 0.1 * randn(n, 17 * 376 + 17)` from generator seed 3000 + n, and
health index 0 with that file's healthy range (-Z, Z) per n. n = 15 is the
first 15 members of params(16) with the Z of n = 16 (a member's episode does
not depend on its neighbours). The eager reference gives these lengths, so
every terminating case but (n = 1, T = 3) kills some members:

    n = 1:  T = 3 [3],           T = 50 [6]
    n = 15: T = 3 two of 2,      T = 50 2 .. 31
    n = 16: T = 3 three of 2,    T = 50 2 .. 31
    n = 17: T = 3 1 .. 3,        T = 50 1 .. 6
    n = 33: T = 3 1 .. 3,        T = 50 1 .. 7

What a kernel other than v7 does with an image: `rollout_env_image_v7` itself
REJECTS a geometry other than the Humanoid one (there is no v7 layout for
it), and a launch that runs v6 or m7 checks the image operand like any other
(device, dtype, size) and then IGNORES it.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

SEED = 41
O, A, R = 376, 17, 16
NS = [1, 15, 16, 17, 33]  # a lone member, partial last blocks, exactly one block, one block plus one member
STEPS = [3, 50]
Z = {1: 0.499, 15: 0.727, 16: 0.727, 17: 0.386, 33: 0.349}  # TABLE[(0, n)] of the terminating test
# column -> c: on the +-15 clamp of tanh_fast, beyond it, and 0 (tests/test_gpu_rollout_v7_packed.py)
CLAMP_C = {0: 20.0, 1: -20.0, 2: 15.0, 3: -15.0, 4: 0.0, 47: -15.0, 48: 20.0, 200: 15.0, 201: 0.0, 375: -20.0}


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


@pytest.fixture(autouse=True)
def _default_kernel(monkeypatch):
    monkeypatch.delenv("EVOTORCH_AMD_ROLLOUT_V6", raising=False)


@functools.lru_cache(maxsize=None)
def _spec(policy_hidden=0):
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    return SyntheticEnvSpec(policy_hidden=policy_hidden)


@functools.lru_cache(maxsize=None)
def _norm():
    g = torch.Generator().manual_seed(7)
    mean = 0.3 * torch.randn(O, generator=g)
    std = 0.5 + torch.rand(O, generator=g)
    return mean, std


@functools.lru_cache(maxsize=None)
def _params(n):
    """On the GPU; callers must not modify it."""
    source = 16 if n == 15 else n
    g = torch.Generator().manual_seed(3000 + source)
    return (0.1 * torch.randn(source, A * O + A, generator=g))[:n].cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _blob(kind="stock"):
    """The environment blob on the GPU (callers must not modify it); "clamp"
    overwrites CLAMP_C's entries of c (blob layout: V [R][O], U_T [R][O],
    D2_T [A][O], c [O], wr, mean, std)."""
    mean, std = _norm()
    blob = _spec().env_blob(mean.cuda(), std.cuda(), device="cuda")
    if kind == "clamp":
        c0 = (2 * R + A) * O
        for col, value in CLAMP_C.items():
            blob[c0 + col] = value
    return blob


@functools.lru_cache(maxsize=None)
def _image(C, kind="stock"):
    return C.rollout_env_image_v7(_blob(kind), O, A, R)


def run_linear(C, params, steps, image, kind="stock", hidden=0):
    spec = _spec()
    stats = torch.zeros(2 * O, device="cuda")
    fit = C.rollout_linear(params, _blob(kind), stats, O, A, R, steps, spec.alive_bonus, spec.act_cost, SEED, 0,
                           hidden, None, image)
    return fit.cpu(), stats.cpu()


def run_terminating(C, params, steps, z, image):
    spec = _spec()
    stats = torch.zeros(2 * O, device="cuda")
    lengths = torch.full((params.shape[0],), -1, dtype=torch.int32, device="cuda")
    fit = C.rollout_terminating(params, _blob(), stats, lengths, O, A, R, steps, spec.alive_bonus, spec.act_cost,
                                SEED, 0, 0, 0, -z, z, None, image)
    return fit.cpu(), stats.cpu(), lengths.cpu()


@requires_gpu
class TestImageAgainstPlainLaunch:
    @pytest.mark.parametrize("steps", STEPS)
    @pytest.mark.parametrize("n", NS)
    def test_rollout_linear(self, C, n, steps):
        assert C.rollout_kernel_name(O, A, R, 0, False) == "v7"
        plain = run_linear(C, _params(n), steps, None)
        imaged = run_linear(C, _params(n), steps, _image(C))
        assert torch.isfinite(plain[0]).all() and torch.isfinite(plain[1]).all()
        for name, x, y in zip(("fitness", "stats"), plain, imaged):
            assert torch.equal(x, y), (name, n, steps)

    @pytest.mark.parametrize("steps", STEPS)
    @pytest.mark.parametrize("n", NS)
    def test_rollout_terminating(self, C, n, steps):
        assert C.rollout_kernel_name(O, A, R, 0, True) == "v7"
        plain = run_terminating(C, _params(n), steps, Z[n], None)
        imaged = run_terminating(C, _params(n), steps, Z[n], _image(C))
        lengths = plain[2]
        print(f"n={n} T={steps}: lengths {lengths.tolist()}")
        assert bool(((lengths >= 1) & (lengths <= steps)).all())
        if (n, steps) != (1, 3):
            assert int(lengths.min()) < steps  # the range kills some members
        assert torch.isfinite(plain[0]).all() and torch.isfinite(plain[1]).all()
        for name, x, y in zip(("fitness", "stats", "lengths"), plain, imaged):
            assert torch.equal(x, y), (name, n, steps)

    @pytest.mark.parametrize("n", [16, 19])  # full-block body alone; full-block and masked body
    def test_clamped_columns(self, C, n):
        params = _params(33)[:n].contiguous()
        plain = run_linear(C, params, 3, None, kind="clamp")
        imaged = run_linear(C, params, 3, _image(C, "clamp"), kind="clamp")
        fit, stats = plain
        assert torch.isfinite(fit).all() and torch.isfinite(stats).all()
        # the environment does what it is for: |c| = 20 saturates the column in every step
        count = 3.0 * n
        for col, value in CLAMP_C.items():
            if abs(value) == 20.0:
                assert abs(stats[col].item() - math.copysign(count, value)) <= count * 2.0**-20, col
        assert torch.equal(plain[0], imaged[0]) and torch.equal(plain[1], imaged[1])
        # and the image matters: the stock image on the clamp blob computes something else
        stock = run_linear(C, params, 3, _image(C), kind="clamp")
        assert not torch.equal(stock[1], plain[1])


@requires_gpu
class TestImage:
    def test_same_blob_same_bytes(self, C):
        first = C.rollout_env_image_v7(_blob(), O, A, R)
        second = C.rollout_env_image_v7(_blob(), O, A, R)
        assert first.dtype == torch.uint8 and first.is_cuda and first.dim() == 1
        assert first.numel() % 16 == 0 and first.data_ptr() % 16 == 0
        assert first.data_ptr() != second.data_ptr()
        assert torch.equal(first, second)

    def test_independent_of_mean_and_std(self, C):
        blob = _blob().clone()
        blob[-2 * O:] = 3.0
        assert torch.equal(C.rollout_env_image_v7(blob, O, A, R), _image(C))

    def test_wrong_size_raises(self, C):
        image = _image(C)
        for bad in (image[:-16].contiguous(), torch.cat([image, image[:16]])):
            with pytest.raises(RuntimeError, match="env_image"):
                run_linear(C, _params(16), 3, bad)
            with pytest.raises(RuntimeError, match="env_image"):
                run_terminating(C, _params(16), 3, Z[16], bad)

    def test_wrong_device_or_dtype_raises(self, C):
        image = _image(C)
        with pytest.raises(RuntimeError, match="env_image"):
            run_linear(C, _params(16), 3, image.cpu())
        with pytest.raises(RuntimeError, match="env_image"):
            run_terminating(C, _params(16), 3, Z[16], image.cpu())
        with pytest.raises(RuntimeError, match="env_image"):
            run_linear(C, _params(16), 3, image.to(torch.int8))

    def test_checks_come_before_the_launch(self, C):
        sentinel = -7.0
        spec = _spec()
        stats = torch.full((2 * O,), sentinel, device="cuda")
        with pytest.raises(RuntimeError, match="env_image"):
            C.rollout_linear(_params(16), _blob(), stats, O, A, R, 3, spec.alive_bonus, spec.act_cost, SEED, 0, 0,
                             None, _image(C)[:-16].contiguous())
        assert bool((stats == sentinel).all())

    def test_other_geometry_is_rejected(self, C):
        from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

        small = SyntheticEnvSpec(obs_dim=32, act_dim=8, rank=8)
        blob = small.env_blob(torch.zeros(32), torch.ones(32), device="cuda")
        with pytest.raises(RuntimeError, match="Humanoid"):
            C.rollout_env_image_v7(blob, 32, 8, 8)
        with pytest.raises(RuntimeError, match="env_blob"):
            C.rollout_env_image_v7(_blob()[:-1].contiguous(), O, A, R)
        with pytest.raises(RuntimeError, match="env_blob"):
            C.rollout_env_image_v7(_blob().cpu(), O, A, R)

    def test_v6_ignores_the_image(self, C, monkeypatch):
        # an image of the right size that holds nothing useful: v6 stages the blob itself
        garbage = torch.full_like(_image(C), 0xFF)
        monkeypatch.setenv("EVOTORCH_AMD_ROLLOUT_V6", "1")
        assert C.rollout_kernel_name(O, A, R, 0, False) == "v6"
        plain = run_linear(C, _params(17), 3, None)
        imaged = run_linear(C, _params(17), 3, garbage)
        assert torch.equal(plain[0], imaged[0]) and torch.equal(plain[1], imaged[1])
        plain_t = run_terminating(C, _params(17), 3, Z[17], None)
        imaged_t = run_terminating(C, _params(17), 3, Z[17], garbage)
        for x, y in zip(plain_t, imaged_t):
            assert torch.equal(x, y)

    def test_m7_ignores_the_image(self, C):
        garbage = torch.full_like(_image(C), 0xFF)
        assert C.rollout_kernel_name(O, A, R, 64, False) == "m7"
        g = torch.Generator().manual_seed(77)
        params = (0.1 * torch.randn(3, _spec(64).solution_length, generator=g)).cuda().contiguous()
        plain = run_linear(C, params, 3, None, hidden=64)
        imaged = run_linear(C, params, 3, garbage, hidden=64)
        assert torch.equal(plain[0], imaged[0]) and torch.equal(plain[1], imaged[1])


def _evaluate(problem, n):
    from evotorch_amd.core import SolutionBatch

    batch = SolutionBatch(problem, popsize=n, empty=True)
    batch.set_values(_params(n).to(problem.device))
    problem.evaluate(batch)
    return batch.evals[:, 0].clone()


@requires_gpu
class TestProblemPassesTheImage:
    @pytest.mark.parametrize("terminating", [False, True])
    def test_one_image_per_problem(self, C, monkeypatch, terminating):
        from evotorch_amd.neuroevolution import SyntheticRolloutProblem

        entry = "rollout_terminating" if terminating else "rollout_linear"
        real = getattr(C, entry)
        seen = []

        def spy(*args):
            seen.append(args[-1])
            return real(*args)

        monkeypatch.setattr(C, entry, spy)
        kwargs = dict(device="cuda:0", seed=5, episode_length=3)
        if terminating:
            kwargs["healthy_range"] = (-Z[17], Z[17])
        first = SyntheticRolloutProblem(env_seed=1234, **kwargs)
        other = SyntheticRolloutProblem(env_seed=4321, **kwargs)
        _evaluate(first, 17)
        _evaluate(first, 17)
        _evaluate(other, 17)
        assert len(seen) == 3
        for image in seen:
            assert isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and image.is_cuda
        # the same tensor in both evaluations of a problem, another one for another environment
        assert seen[0] is seen[1]
        assert seen[0].shape == seen[2].shape and not torch.equal(seen[0], seen[2])
        # it is the image of the problem's own blob
        blob = first.spec.env_blob(torch.zeros(O), torch.ones(O), device="cuda")
        assert torch.equal(seen[0], C.rollout_env_image_v7(blob, O, A, R))

    def test_problem_results_do_not_depend_on_the_image(self, C, monkeypatch):
        from evotorch_amd.neuroevolution import SyntheticRolloutProblem

        def evaluate_twice():
            problem = SyntheticRolloutProblem(device="cuda:0", seed=5, episode_length=3)
            return _evaluate(problem, 33), _evaluate(problem, 33), problem.obs_norm.mean.clone()

        with_image = evaluate_twice()
        monkeypatch.setattr(SyntheticRolloutProblem, "_env_image", lambda self, mod, blob: None)
        without = evaluate_twice()
        for x, y in zip(with_image, without):
            assert torch.equal(x, y)

    def test_v6_problem_gets_no_image(self, C, monkeypatch):
        from evotorch_amd.neuroevolution import SyntheticRolloutProblem

        real = C.rollout_linear
        seen = []

        def spy(*args):
            seen.append(args[-1])
            return real(*args)

        monkeypatch.setattr(C, "rollout_linear", spy)
        monkeypatch.setenv("EVOTORCH_AMD_ROLLOUT_V6", "1")
        _evaluate(SyntheticRolloutProblem(device="cuda:0", seed=5, episode_length=3), 17)
        assert seen == [None]
