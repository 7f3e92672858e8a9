"""Packed GEMM2 epilogue of the v7 rollout kernel (linear policy, Humanoid geometry).

The epilogue works on the four member rows of a lane's MFMA result as two
pairs (r, r+1) in two-wide fp32 instructions. These tests pin down what the
pairing must not change:

1. a member of a partial block has the bits of a one-member launch, whether
   its pair partner is live or dead (the last block holds 1, 2, 3 or 15 live
   members, so a pair is cut at every position),
2. fitness, sum and sumsq of those populations equal the bits recorded from
   the kernel before the epilogue was packed,
3. the same for an environment whose `c` puts pre-activations on and beyond
   the +-15 clamp of tanh_fast in a handful of columns: the stock environment
   never reaches the clamp, so no other recorded case has a clamped value
   next to packed neighbours.

tests/golden/rollout_v7_bits_packed.npz is written by
scripts/record_rollout_v7_bits_packed.py on an MI355X.
"""

import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

SEED = 41
A, O = 17, 376
N_MAX = 31
STEPS = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_v7_bits_packed.npz")
BOUNDARY_NS = [17, 18, 19, 31]   # 1, 2, 3 and 15 live members in the last block
CLAMP_NS = [16, 19]              # full-block body alone; full-block and masked body
# column -> c: on the clamp, beyond it, and 0, next to stock columns, in the
# first and the last tile of a wave and in the last real column
CLAMP_C = {0: 20.0, 1: -20.0, 2: 15.0, 3: -15.0, 4: 0.0, 47: -15.0, 48: 20.0, 200: 15.0, 201: 0.0, 375: -20.0}
# (kind, n) of every recorded case
GOLDEN_CASES = [("stock", n) for n in BOUNDARY_NS] + [("clamp", n) for n in CLAMP_NS]


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


@pytest.fixture(autouse=True)
def _default_kernel(monkeypatch):
    monkeypatch.delenv("EVOTORCH_AMD_ROLLOUT_V6", raising=False)


@functools.lru_cache(maxsize=None)
def _spec():
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    return SyntheticEnvSpec(episode_length=STEPS)


@functools.lru_cache(maxsize=None)
def _norm():
    """The layout test's non-trivial observation normalization."""
    g = torch.Generator().manual_seed(7)
    mean = 0.3 * torch.randn(O, generator=g)
    std = 0.5 + torch.rand(O, generator=g)
    return mean, std


@functools.lru_cache(maxsize=None)
def _params():
    """A case with members [lo, hi) uses rows [lo, hi), so the same member has
    the same weights in every case."""
    g = torch.Generator().manual_seed(1000 + N_MAX)
    return 0.1 * torch.randn(N_MAX, A * O + A, generator=g)


@functools.lru_cache(maxsize=None)
def _blob(kind):
    """The environment blob on the GPU (callers must not modify it); "clamp"
    overwrites CLAMP_C's entries of c (blob layout: V [R][O], U_T [R][O],
    D2_T [A][O], c [O], ...)."""
    spec = _spec()
    mean, std = _norm()
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    if kind == "clamp":
        c0 = (2 * spec.rank + spec.act_dim) * spec.obs_dim
        for col, value in CLAMP_C.items():
            blob[c0 + col] = value
    return blob


def run_kernel(C, kind, lo, hi):
    """Members [lo, hi) as one launch with member_offset = lo."""
    spec = _spec()
    stats = torch.zeros(2 * O, device="cuda")
    fit = C.rollout_linear(_params()[lo:hi].cuda().contiguous(), _blob(kind), stats, spec.obs_dim, spec.act_dim,
                           spec.rank, STEPS, spec.alive_bonus, spec.act_cost, SEED, lo)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu()


@functools.lru_cache(maxsize=None)
def _cached_run(C, kind, n):
    return run_kernel(C, kind, 0, n)


@functools.lru_cache(maxsize=None)
def _single(C, m):
    return run_kernel(C, "stock", m, m + 1)[0]


@requires_gpu
class TestPackedEpilogue:
    @pytest.mark.parametrize("n", BOUNDARY_NS)
    def test_partial_block_members_equal_single_member_shards(self, C, n):
        fit, _, _ = _cached_run(C, "stock", n)
        for m in range(16, n):
            assert torch.equal(fit[m:m + 1], _single(C, m)), (n, m, fit[m], _single(C, m))

    @pytest.mark.parametrize("kind,n", GOLDEN_CASES)
    def test_bits_unchanged(self, C, kind, n):
        golden = np.load(GOLDEN)
        got_all = _cached_run(C, kind, n)
        for name, got in zip(("fitness", "sum", "sumsq"), got_all):
            want = torch.from_numpy(golden[f"{name}_{kind}_n{n}"])
            assert torch.isfinite(got).all(), name
            print(f"{kind} n={n} {name}: max|d|={(got - want).abs().max():.3e}")
            assert torch.equal(got, want), name

    @pytest.mark.parametrize("n", CLAMP_NS)
    def test_clamped_columns_saturate(self, C, n):
        """The inputs do what they are for: with |c| = 20 the pre-activation
        of the column is beyond the clamp for every member in all STEPS steps
        (the GEMM terms stay within a few units), so each value is
        tanh_fast(+-15). That is (e - 1) * rcp(e + 1) with e = 2^+-43: e -+ 1
        rounds to e or to -+1, so the value is +-1 up to the 1 ulp of v_rcp_f32
        and the rounding of the product, under 2^-22. Column sum and sumsq are
        STEPS*n such values; 2^-20 relative leaves room for their own
        roundings (STEPS*n <= 57 adds of 2^-24 each). All values are finite."""
        fit, s, sq = _cached_run(C, "clamp", n)
        assert torch.isfinite(fit).all() and torch.isfinite(s).all() and torch.isfinite(sq).all()
        count = float(STEPS * n)
        for col, value in CLAMP_C.items():
            if abs(value) == 20.0:
                print(f"n={n} col={col}: sum={s[col].item()!r} sumsq={sq[col].item()!r}")
                assert abs(s[col].item() - (count if value > 0 else -count)) <= count * 2.0**-20, (col, s[col])
                assert abs(sq[col].item() - count) <= count * 2.0**-20, (col, sq[col])
