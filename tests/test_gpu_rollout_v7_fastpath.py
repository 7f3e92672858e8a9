"""Full-block fast path of the v7 rollout kernel (linear policy, Humanoid geometry).

A block whose 16 member slots are all live runs a loop body without the
per-member guards; a partial block runs the masked body. Both must give a
member the same bits, match `rollout_eager`, and reproduce the outputs
recorded from the kernel before the fast path existed
(tests/golden/rollout_v7_bits.npz: this project's own fitness, sum and sumsq
for (n, T) = (17, 3) and (16, 1), recorded on an MI355X).
"""

import functools
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
N_MAX = 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_v7_bits.npz")
GOLDEN_CASES = [(17, 3), (16, 1)]


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
def _all_params():
    """"plain" parameters; a case with n members uses rows [0, n), so the
    same member has the same weights in every case."""
    g = torch.Generator().manual_seed(1000 + N_MAX)
    return 0.1 * torch.randn(N_MAX, A * O + A, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(n, steps):
    """CPU reference, computed once per case and shared (callers must not modify it)."""
    from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

    mean, std = _norm()
    fit, (_, s, sq) = rollout_eager(_spec(steps), _all_params()[:n], mean, std, init_seed=SEED)
    assert torch.isfinite(fit).all() and torch.isfinite(s).all() and torch.isfinite(sq).all()
    return fit, s, sq


def run_kernel(C, lo, hi, steps):
    """Members [lo, hi) as one launch with member_offset = lo."""
    spec = _spec(steps)
    mean, std = _norm()
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.zeros(2 * O, device="cuda")
    params = _all_params()[lo:hi].cuda().contiguous()
    fit = C.rollout_linear(params, blob, stats, spec.obs_dim, spec.act_dim, spec.rank,
                           steps, spec.alive_bonus, spec.act_cost, SEED, lo)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu()


@functools.lru_cache(maxsize=None)
def _cached_run(C, n, steps):
    return run_kernel(C, 0, n, steps)


@requires_gpu
class TestFastPath:
    # 16, 32: full blocks only; 17: a full block and a one-member block; 5: one partial block
    @pytest.mark.parametrize("n,steps", [(16, 1), (16, 3), (17, 3), (5, 3), (32, 2)])
    def test_matches_eager(self, C, n, steps):
        fit, s, sq = _cached_run(C, n, steps)
        efit, es, esq = _reference(n, steps)
        print(f"n={n} T={steps}: max|dfit|={(fit - efit).abs().max():.3e} "
              f"max|dsum|={(s - es).abs().max():.3e} max|dsumsq|={(sq - esq).abs().max():.3e}")
        assert torch.allclose(fit, efit, **FIT_TOL), (fit, efit)
        assert torch.allclose(s, es, **STAT_TOL)
        assert torch.allclose(sq, esq, **STAT_TOL)

    def test_full_body_equals_masked_body(self, C):
        full, _, _ = _cached_run(C, 16, 3)
        masked, _, _ = _cached_run(C, 5, 3)
        assert torch.equal(full[0:5], masked)

    def test_last_member_equals_single_member_shard(self, C):
        both, _, _ = _cached_run(C, 17, 3)
        one, _, _ = run_kernel(C, 16, 17, 3)
        assert torch.equal(both[16:17], one)

    @pytest.mark.parametrize("n,steps", [(16, 3), (32, 2)])
    def test_statistics_repeatable(self, C, n, steps):
        _, s0, sq0 = _cached_run(C, n, steps)
        _, s1, sq1 = run_kernel(C, 0, n, steps)
        assert torch.equal(s0, s1)
        assert torch.equal(sq0, sq1)

    @pytest.mark.parametrize("n,steps", GOLDEN_CASES)
    def test_bits_unchanged(self, C, n, steps):
        golden = np.load(GOLDEN)
        fit, s, sq = _cached_run(C, n, steps)
        for name, got in (("fitness", fit), ("sum", s), ("sumsq", sq)):
            want = torch.from_numpy(golden[f"{name}_n{n}_t{steps}"])
            print(f"n={n} T={steps} {name}: max|d|={(got - want).abs().max():.3e}")
            assert torch.equal(got, want), name
