"""Layout checks for the v7 rollout kernel (linear policy, Humanoid geometry).

The kernel reduces the 16+1 policy accumulators with a transposing
butterfly (a lane ends up owning one action), runs the action tail once on
17 lanes and folds Σa² from actions exchanged through LDS; GEMM2 hands
each lane one obs column of four members. Every case here compares `_C.rollout_linear` with `rollout_eager` (run on
the CPU) on short episodes, chosen so that a transposed action, a wrong
member/column owner, a dead lane leaking into the statistics or a
slot-dependent summation shows up.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

# tolerances of TestRollout.test_matches_eager_reference
FIT_TOL = dict(rtol=2e-2, atol=2e-2)
STAT_TOL = dict(rtol=5e-2, atol=5e-1)
SEED = 41
A, O = 17, 376


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
    """Non-trivial observation normalization shared by every case."""
    g = torch.Generator().manual_seed(7)
    mean = 0.3 * torch.randn(O, generator=g)
    std = 0.5 + torch.rand(O, generator=g)
    return mean, std


@functools.lru_cache(maxsize=None)
def _params(kind, n):
    g = torch.Generator().manual_seed(1000 + n)
    L = A * O + A
    if kind == "plain":
        return 0.1 * torch.randn(n, L, generator=g)
    if kind == "one_row":
        # member m: only row m % 17 of W is non-zero; distinct biases per action
        p = torch.zeros(n, L)
        W = p[:, : A * O].view(n, A, O)
        for m in range(n):
            W[m, m % A] = 0.05 * torch.randn(O, generator=g)
        p[:, A * O :] = (torch.arange(A, dtype=torch.float32) - 8.0) / 8.0
        return p
    if kind == "saturated":
        p = 0.3 * torch.randn(n, L, generator=g)
        # member 3: W = 0 and |b| > 1, every action is exactly ±1 at every step
        p[3, : A * O] = 0.0
        p[3, A * O :] = 1.5 * (1.0 - 2.0 * (torch.arange(A) % 2).to(torch.float32))
        return p
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _reference(kind, n, steps):
    """CPU reference, computed once per case and shared (callers must not modify it)."""
    from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

    mean, std = _norm()
    fit, (_, s, sq) = rollout_eager(_spec(steps), _params(kind, n), mean, std, init_seed=SEED)
    assert torch.isfinite(fit).all() and torch.isfinite(s).all() and torch.isfinite(sq).all()
    return fit, s, sq


def _run(C, params, steps, member_offset=0):
    spec = _spec(steps)
    mean, std = _norm()
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.zeros(2 * O, device="cuda")
    fit = C.rollout_linear(params.cuda().contiguous(), blob, stats, spec.obs_dim, spec.act_dim, spec.rank,
                           steps, spec.alive_bonus, spec.act_cost, SEED, member_offset)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu()


def _check(C, kind, n, steps):
    fit, s, sq = _run(C, _params(kind, n), steps)
    efit, es, esq = _reference(kind, n, steps)
    print(f"{kind} n={n} T={steps}: max|dfit|={(fit - efit).abs().max():.3e} "
          f"max|dsum|={(s - es).abs().max():.3e} max|dsumsq|={(sq - esq).abs().max():.3e}")
    assert torch.allclose(fit, efit, **FIT_TOL), (fit, efit)
    assert torch.allclose(s, es, **STAT_TOL)
    assert torch.allclose(sq, esq, **STAT_TOL)
    return fit, efit


@requires_gpu
class TestBlocks:
    # n = 17: the second block has one live member, its 15 dead lanes must stay out of the stats
    @pytest.mark.parametrize("n", [1, 7, 16, 17, 33])
    def test_partial_and_multiple_blocks(self, C, n):
        _, efit = _check(C, "plain", n, 8)
        if n > 1:
            assert efit.std() > 10 * FIT_TOL["atol"]  # the members are told apart


@requires_gpu
class TestSingleSteps:
    # T = 1 tests GEMM2 from the philox initial observations, T = 2 the
    # written-back obs/obsn, before bf16 rounding flips can compound.
    # Bound: twice the maximum |fitness - eager| of the kernel BEFORE the
    # transposing reduction on these inputs (at most the fp32 summation
    # order may change).
    # Measured on MI355X for that kernel: T=1 1.1921e-07, T=2 7.4863e-05.
    PARENT_MAX_DEV = {1: 1.1921e-07, 2: 7.4863e-05}

    @pytest.mark.parametrize("steps", [1, 2])
    def test_short_episode_fitness(self, C, steps):
        fit, _, _ = _run(C, _params("plain", 16), steps)
        efit, _, _ = _reference("plain", 16, steps)
        dev = (fit - efit).abs().max().item()
        print(f"T={steps}: max|dfit|={dev:.3e} bound={2 * self.PARENT_MAX_DEV[steps]:.3e}")
        assert dev <= 2 * self.PARENT_MAX_DEV[steps]
        _check(C, "plain", 16, steps)


@requires_gpu
class TestActions:
    # T = 1 bound for the action case. Against the eager reference the
    # kernel differs by fp32 summation order (< 1e-5 on a fitness of ~1)
    # and, rarely, by a bf16 rounding that falls the other way: of an h
    # value (|h| < 0.42 here, so 0.42 * 2^-8, times max|U wr| = 0.46:
    # 7.5e-4) or of an action (2^-8, times max|D2 wr| = 0.25: 1e-3; tanh'
    # <= 1). The bound admits two such flips in one member.
    ACTION_ATOL_T1 = 2e-3

    def test_action_indexing(self, C):
        """One non-zero W row per member and distinct biases: a permuted or
        transposed action (action 16 on the rank-1 path included) moves the
        fitness far outside the bound. 34 members put every action row in
        two different block slots."""
        from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

        n = 34
        fit, _, _ = _run(C, _params("one_row", n), 1)
        efit, _, _ = _reference("one_row", n, 1)
        print(f"one_row T=1: max|dfit|={(fit - efit).abs().max():.3e}")
        assert (fit - efit).abs().max() <= self.ACTION_ATOL_T1
        # the case can tell: rotating the actions by one moves every member by > 10 bounds
        p = _params("one_row", n).clone()
        p[:, : A * O] = p[:, : A * O].view(n, A, O).roll(1, dims=1).reshape(n, -1)
        p[:, A * O :] = p[:, A * O :].roll(1, dims=1)
        mean, std = _norm()
        rfit, _ = rollout_eager(_spec(1), p, mean, std, init_seed=SEED)
        assert ((rfit - efit).abs() > 10 * self.ACTION_ATOL_T1).all()
        _check(C, "one_row", n, 4)

    def test_saturation(self, C):
        """Member 3 has W = 0 and |b| > 1: its actions are exactly ±1, so its
        Σa² and action cost are exact."""
        n, steps = 16, 8
        _check(C, "saturated", n, steps)
        # a good share of the actions clamp
        spec, (mean, std) = _spec(steps), _norm()
        p = _params("saturated", n)
        obs0 = spec.initial_obs(n, 0, SEED).to(torch.bfloat16).float()
        obsn = ((obs0 - mean) / std).to(torch.bfloat16).float()
        W = p[:, : A * O].view(n, A, O).to(torch.bfloat16).float()
        pre = torch.einsum("nao,no->na", W, obsn) + p[:, A * O :]
        assert (pre.abs() > 1).float().mean() > 0.3


@requires_gpu
class TestDeterminism:
    def test_bitwise_repeatable(self, C):
        a = _run(C, _params("plain", 33), 10)
        b = _run(C, _params("plain", 33), 10)
        for x, y in zip(a, b):
            assert torch.equal(x, y)

    @pytest.mark.parametrize("k", [1, 8, 15])
    def test_slot_invariance(self, C, k):
        """Rows [k:] run with member_offset = k land in other block slots
        (other half-wave, other wave, other block) and must not change."""
        p = _params("plain", 33)
        full, _, _ = _run(C, p, 10)
        shard, _, _ = _run(C, p[k:], 10, member_offset=k)
        assert torch.equal(full[k:], shard)
