"""Select-free policy butterfly of the v7 rollout kernel (linear policy, Humanoid geometry).

A lane of the kernel accumulates action `a ^ perm(lane)` in accumulator
register `a` (the weight rows are loaded permuted, once), so that every level
of the transposing reduction is one add. These tests pin down what that must
not change:

1. each of the 17 weight rows still drives its own action (a wrong row
   permutation shows as a swapped action),
2. a member's bits do not depend on its slot (half-wave, wave, block, full or
   masked loop body),
3. fitness, sum and sumsq of 50-step episodes equal the bits recorded from the
   kernel before the change (tests/golden/rollout_v7_bits_t50.npz, written by
   scripts/record_rollout_v7_bits_t50.py on an MI355X): 50 closed-loop steps
   let a one-ulp difference in an action or a statistic surface.
"""

import functools
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

# tolerances of tests/test_gpu_rollout_v7_layout.py (TestRollout.test_matches_eager_reference)
FIT_TOL = dict(rtol=2e-2, atol=2e-2)
STAT_TOL = dict(rtol=5e-2, atol=5e-1)
SEED = 41
A, O = 17, 376
N_MAX = 33
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_v7_bits_t50.npz")
GOLDEN_CASES = [(16, 50), (17, 50)]
SLOTS = [0, 1, 15, 16, 31, 32]


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


@pytest.fixture(autouse=True)
def _default_kernel(monkeypatch):
    monkeypatch.delenv("EVOTORCH_AMD_ROLLOUT_V6", raising=False)


def _spec(steps):
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    return SyntheticEnvSpec(episode_length=steps)


@functools.lru_cache(maxsize=None)
def _norm():
    """The layout test's non-trivial observation normalization."""
    g = torch.Generator().manual_seed(7)
    mean = 0.3 * torch.randn(O, generator=g)
    std = 0.5 + torch.rand(O, generator=g)
    return mean, std


@functools.lru_cache(maxsize=None)
def _random_params():
    """A case with members [lo, hi) uses rows [lo, hi), so the same member has
    the same weights in every case."""
    g = torch.Generator().manual_seed(1000 + N_MAX)
    return 0.1 * torch.randn(N_MAX, A * O + A, generator=g)


@functools.lru_cache(maxsize=None)
def _one_row_params(a):
    """16 members whose weight matrix is zero except row `a` and whose bias is
    zero except b[a]. Row and bias are a per-member pattern that does not
    depend on `a`: member m's row is scale_m times a fixed +-1 pattern (so the
    dot product with the normalized observation is a few tenths), its bias
    0.75 + 0.01 m, so every member pushes the driven action the same way and
    the observation sums add up over the members. Only WHICH action they
    drive differs between two values of `a`."""
    g = torch.Generator().manual_seed(2024)
    signs = torch.randint(0, 2, (O,), generator=g).float() * 2.0 - 1.0
    m = torch.arange(16, dtype=torch.float32)
    scale = 0.02 + 0.004 * m
    bias = 0.75 + 0.01 * m
    params = torch.zeros(16, A * O + A)
    params[:, a * O:(a + 1) * O] = scale[:, None] * signs[None, :]
    params[:, A * O + a] = bias
    return params


def run_kernel(C, params, steps, member_offset=0):
    """One launch over the rows of `params`, global member ids starting at member_offset."""
    spec = _spec(steps)
    mean, std = _norm()
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.zeros(2 * O, device="cuda")
    fit = C.rollout_linear(params.cuda().contiguous(), blob, stats, spec.obs_dim, spec.act_dim, spec.rank,
                           steps, spec.alive_bonus, spec.act_cost, SEED, member_offset)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu()


def run_eager(params, steps):
    from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

    mean, std = _norm()
    fit, (_, s, sq) = rollout_eager(_spec(steps), params, mean, std, init_seed=SEED)
    assert torch.isfinite(fit).all() and torch.isfinite(s).all() and torch.isfinite(sq).all()
    return fit, s, sq


@functools.lru_cache(maxsize=None)
def _one_row_reference():
    """rollout_eager for the 17 one-row populations, computed once (callers
    must not modify it). Also checks a property of the inputs themselves:
    driving action b instead of a moves a fitness or a column sum by more
    than four times the tolerance the kernel is compared at, so a swapped
    pair of actions cannot pass test_each_row_drives_its_action."""
    ref = [run_eager(_one_row_params(a), 1) for a in range(A)]
    for a, b in itertools.combinations(range(A), 2):
        apart = False
        for x, y, tol in zip(ref[a], ref[b], (FIT_TOL, STAT_TOL, STAT_TOL)):
            bound = tol["atol"] + tol["rtol"] * torch.maximum(x.abs(), y.abs())
            apart = apart or bool(((x - y).abs() > 4.0 * bound).any())
        assert apart, (a, b)
    return ref


@functools.lru_cache(maxsize=None)
def _one_row_kernel(C):
    return [run_kernel(C, _one_row_params(a), 1) for a in range(A)]


@functools.lru_cache(maxsize=None)
def _cached_random_run(C, n, steps):
    return run_kernel(C, _random_params()[:n], steps)


@requires_gpu
class TestButterfly:
    @pytest.mark.parametrize("a", range(A))
    def test_each_row_drives_its_action(self, C, a):
        fit, s, sq = _one_row_kernel(C)[a]
        efit, es, esq = _one_row_reference()[a]
        print(f"a={a}: max|dfit|={(fit - efit).abs().max():.3e} "
              f"max|dsum|={(s - es).abs().max():.3e} max|dsumsq|={(sq - esq).abs().max():.3e}")
        assert torch.allclose(fit, efit, **FIT_TOL), (fit, efit)
        assert torch.allclose(s, es, **STAT_TOL)
        assert torch.allclose(sq, esq, **STAT_TOL)

    def test_actions_differ_pairwise(self, C):
        runs = _one_row_kernel(C)
        for a, b in itertools.combinations(range(A), 2):
            for name, x, y in zip(("fitness", "sum", "sumsq"), runs[a], runs[b]):
                assert not torch.equal(x, y), (a, b, name)

    @pytest.mark.parametrize("m", SLOTS)
    def test_every_slot_equals_single_member_shard(self, C, m):
        """n = 33: both half-waves, first and last wave of the full blocks, and
        the masked body (member 32); the one-member launch runs the masked
        body in slot 0."""
        every, _, _ = _cached_random_run(C, N_MAX, 3)
        one, _, _ = run_kernel(C, _random_params()[m:m + 1], 3, member_offset=m)
        assert torch.equal(every[m:m + 1], one), (m, every[m], one)

    @pytest.mark.parametrize("n,steps", GOLDEN_CASES)
    def test_long_episode_bits_unchanged(self, C, n, steps):
        golden = np.load(GOLDEN)
        fit, s, sq = _cached_random_run(C, n, steps)
        for name, got in (("fitness", fit), ("sum", s), ("sumsq", sq)):
            want = torch.from_numpy(golden[f"{name}_n{n}_t{steps}"])
            print(f"n={n} T={steps} {name}: max|d|={(got - want).abs().max():.3e}")
            assert torch.equal(got, want), name
