"""Checks for the general (v6) rollout kernel: any geometry, linear or MLP policy.

The default Humanoid geometry routes to the specialised v7 / m7 kernels, so
every case here is either off that geometry or forces v6 with
EVOTORCH_AMD_ROLLOUT_V6. Each shape is the smallest that reaches the named
path of the kernel; every case compares `_C.rollout_linear` with
`rollout_eager` (run on the CPU) on a 4-step episode.
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
STEPS = 4

# (obs_dim, act_dim, rank, policy_hidden, force_v6)
CASES = {
    # 16 obs pairs = two full 8-lane iterations, no tail
    "linear_base": (32, 8, 8, 0, False),
    # odd A and R (zero-padded A_PAD/R_PAD pairs); 10 obs pairs = one full
    # iteration (the `full_iters & 1` branch) plus a 2-lane tail
    "linear_odd": (20, 3, 5, 0, False),
    # MLP phase B with 3 hidden pairs: tail-only dot
    "mlp_tail_only": (20, 3, 5, 6, False),
    # MLP, one full iteration in phase B
    "mlp_base": (32, 8, 8, 16, False),
    # members*O = 600 > 512 threads: second pass of the dynamics loop, second stat slot
    "wide_obs": (300, 4, 4, 0, False),
    # two members need 200,600 B of LDS (> 160 KB): one-member-per-block fallback
    "one_member": (376, 17, 16, 96, False),
    # v6 at the geometry v7 and m7 normally take
    "humanoid_linear_v6": (376, 17, 16, 0, True),
    "humanoid_mlp64_v6": (376, 17, 16, 64, True),
}
# n = 1: one block, half-live; n = 5: the last block has one live member
NS = (1, 2, 5)

# max |kernel - eager| over every case and n above, measured on MI355X for the
# kernel as it stood before the shared-helper refactor (the commit that
# introduced this module ran it first on its parent). A later change may move
# these by a changed fp32 contraction at most, hence the factor 2 below.
PARENT_MAX_DEV = {"fitness": 9.536743e-07, "sum": 1.907349e-06, "sumsq": 1.430511e-06}


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


def _spec(case):
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    O, A, R, H, _ = CASES[case]
    return SyntheticEnvSpec(episode_length=STEPS, obs_dim=O, act_dim=A, rank=R, policy_hidden=H)


@functools.lru_cache(maxsize=None)
def _norm(O):
    g = torch.Generator().manual_seed(7)
    mean = 0.3 * torch.randn(O, generator=g)
    std = 0.5 + torch.rand(O, generator=g)
    return mean, std


@functools.lru_cache(maxsize=None)
def _params(case, n):
    g = torch.Generator().manual_seed(2000 + n)
    return 0.1 * torch.randn(n, _spec(case).solution_length, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(case, n):
    """CPU reference, computed once per case and shared (callers must not modify it)."""
    from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

    spec = _spec(case)
    mean, std = _norm(spec.obs_dim)
    fit, (_, s, sq) = rollout_eager(spec, _params(case, n), mean, std, init_seed=SEED)
    assert torch.isfinite(fit).all() and torch.isfinite(s).all() and torch.isfinite(sq).all()
    return fit, s, sq


def _run(C, case, n):
    spec = _spec(case)
    O = spec.obs_dim
    mean, std = _norm(O)
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.zeros(2 * O, device="cuda")
    fit = C.rollout_linear(_params(case, n).cuda().contiguous(), blob, stats, O, spec.act_dim, spec.rank,
                           STEPS, spec.alive_bonus, spec.act_cost, SEED, 0, spec.policy_hidden)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu()


@pytest.fixture
def kernel_env(monkeypatch):
    def select(case):
        if CASES[case][4]:
            monkeypatch.setenv("EVOTORCH_AMD_ROLLOUT_V6", "1")
        else:
            monkeypatch.delenv("EVOTORCH_AMD_ROLLOUT_V6", raising=False)

    return select


@requires_gpu
class TestGeneralKernel:
    @pytest.mark.parametrize("n", NS)
    @pytest.mark.parametrize("case", list(CASES))
    def test_matches_eager(self, C, kernel_env, case, n):
        kernel_env(case)
        fit, s, sq = _run(C, case, n)
        efit, es, esq = _reference(case, n)
        dev = {
            "fitness": (fit - efit).abs().max().item(),
            "sum": (s - es).abs().max().item(),
            "sumsq": (sq - esq).abs().max().item(),
        }
        print(f"{case} n={n}: max|dfit|={dev['fitness']:.4e} max|dsum|={dev['sum']:.4e} "
              f"max|dsumsq|={dev['sumsq']:.4e}")
        if n == 5:
            assert efit.std() > 10 * FIT_TOL["atol"]  # the members are told apart
        for key, d in dev.items():
            assert d <= 2 * PARENT_MAX_DEV[key], (key, d)
        assert torch.allclose(fit, efit, **FIT_TOL), (fit, efit)
        assert torch.allclose(s, es, **STAT_TOL)
        assert torch.allclose(sq, esq, **STAT_TOL)

    def test_bitwise_repeatable(self, C, kernel_env):
        kernel_env("wide_obs")
        a = _run(C, "wide_obs", 5)
        b = _run(C, "wide_obs", 5)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
