"""The generation tail between two rollouts: register/lane bitonic rank,
one-launch ClipUp + sigma update, one-launch obs-norm pack and merge.

Everything here is an equality of bits (`torch.equal`):

* `fused_rank` against a numpy emulator of the serial bitonic network (same
  step order, same swap predicate, index payload), which is itself checked on
  the CPU to be a sort; the nes utilities against outputs recorded from the
  kernel before its data moved into registers (golden/fused_rank_nes.npz).
* `gaussian_clipup_update` against the chain of launches it replaces.
* `obsnorm_pack_` / `obsnorm_merge_` against RunningNorm's torch chains.
* whole PGPE runs with the fused tail against the same runs without it, and
  against arrays recorded from the commit before the fused tail existed
  (golden/generation_tail_e2e.npz, recorded on an MI355X).
"""

import functools
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---------------------------------------------------------------------------
# 1. rank against the network
# ---------------------------------------------------------------------------

RANK_SIZES = [2, 3, 5, 63, 64, 65, 128, 129, 1000, 1024, 1025, 4000, 4096, 4097, 8192]
RANK_KEYS = ["randn", "ties", "equal", "flagship"]


@functools.lru_cache(maxsize=None)
def _fitness(kind, n):
    """fp32 fitness vector, computed once per case (callers must not modify it)."""
    g = torch.Generator().manual_seed(1000 * RANK_KEYS.index(kind) + n)
    if kind == "randn":
        fit = torch.randn(n, generator=g)
    elif kind == "ties":
        fit = torch.randint(0, 8, (n,), generator=g).to(torch.float32)
    elif kind == "equal":
        fit = torch.full((n,), 1.25)
    else:
        # flagship-like: episode returns of a few hundred, a few percent of
        # them equal to another member's
        fit = 400.0 + 35.0 * torch.randn(n, generator=g)
        dup = max(1, n // 25)
        dst = torch.randperm(n, generator=g)[:dup]
        src = torch.randint(0, n, (dup,), generator=g)
        fit[dst] = fit[src]
    return fit.to(torch.float32)


def network_sort(keys):
    """The serial bitonic network on fp32 `keys` padded to a power of two
    with +inf: for k = 2, 4 .. p, for j = k/2 .. 1, compare-exchange
    (i, i ^ j) for every i with (i & j) == 0, ascending where (i & k) == 0.
    The pairs of one step are disjoint, so a step is vectorised. Returns the
    sorted keys and the index payload, both of length p."""
    keys = np.asarray(keys, dtype=np.float32)
    n = keys.shape[0]
    p = 1
    while p < n:
        p <<= 1
    key = np.full(p, np.inf, dtype=np.float32)
    key[:n] = keys
    idx = np.arange(p, dtype=np.int64)
    pos = np.arange(p, dtype=np.int64)
    k = 2
    while k <= p:
        j = k >> 1
        while j > 0:
            lo = pos[(pos & j) == 0]
            hi = lo ^ j
            up = (lo & k) == 0
            a, b = key[lo], key[hi]
            nan_a, nan_b = np.isnan(a), np.isnan(b)
            with np.errstate(invalid="ignore"):
                swap = np.where(up, (b < a) | (nan_a & ~nan_b), (a < b) | (nan_b & ~nan_a))
            s_lo, s_hi = lo[swap], hi[swap]
            key[s_lo], key[s_hi] = b[swap], a[swap]
            idx[s_lo], idx[s_hi] = idx[s_hi].copy(), idx[s_lo].copy()
            j >>= 1
        k <<= 1
    return key, idx


def network_utilities(fit, method, higher_better):
    """What fused_rank's tail writes for methods 0 (centered) and 1
    (linear): position r of the sorted order gets r * inv - 0.5 (one fma:
    the product is exact in fp64 and the difference rounds once) or r * inv,
    inv = 1 / (n - 1) in fp32."""
    fit = np.asarray(fit, dtype=np.float32)
    n = fit.shape[0]
    _, idx = network_sort(fit if higher_better else -fit)
    order = idx[:n]
    assert (order < n).all()  # finite keys: the +inf pad stays behind them
    inv = np.float32(1.0) / np.float32(n - 1) if n > 1 else np.float32(0.0)
    r = np.arange(n, dtype=np.float32)
    if method == 0:
        values = (r.astype(np.float64) * np.float64(inv) - 0.5).astype(np.float32)
    else:
        values = r * inv
    out = np.empty(n, dtype=np.float32)
    out[order] = values
    return out


@pytest.mark.parametrize("kind", RANK_KEYS)
@pytest.mark.parametrize("n", [2, 3, 5, 65, 1000, 4097])
def test_network_emulator_sorts(kind, n):
    """The specification itself, on the CPU: the network is a sort for any
    input, and for distinct keys its order is argsort's."""
    fit = _fitness(kind, n).numpy()
    key, idx = network_sort(fit)
    assert sorted(idx.tolist()) == list(range(len(idx)))
    assert (key[:-1] <= key[1:]).all()
    real = idx[idx < n]
    assert np.array_equal(key[: n], fit[real])
    if len(np.unique(fit)) == n:
        assert np.array_equal(real, np.argsort(fit, kind="stable"))
    for method in (0, 1):
        out = network_utilities(fit, method, True)
        expected_sum = 0.0 if method == 0 else n / 2.0
        assert abs(float(out.astype(np.float64).sum()) - expected_sum) < 1e-3 * n


@gpu
@requires_gpu
@pytest.mark.parametrize("kind", RANK_KEYS)
@pytest.mark.parametrize("n", RANK_SIZES)
def test_fused_rank_equals_network(kind, n):
    import evotorch_amd._C as C

    fit = _fitness(kind, n)
    dev = fit.cuda()
    for higher_better in (True, False):
        for method in (0, 1):
            got = C.fused_rank(dev, method, higher_better).cpu()
            want = torch.from_numpy(network_utilities(fit.numpy(), method, higher_better))
            assert torch.equal(got, want), (n, kind, method, higher_better, int((got != want).sum()))


@gpu
@requires_gpu
@pytest.mark.parametrize("n", [5, 1000, 4000])
def test_fused_rank_nes_equals_recorded(n):
    """nes sums its utilities in the kernel's own order, so its oracle is
    the kernel's output before the sort moved into registers."""
    import evotorch_amd._C as C

    golden = np.load(os.path.join(GOLDEN_DIR, "fused_rank_nes.npz"))
    fit = torch.from_numpy(golden[f"n{n}_fit"])
    assert len(np.unique(golden[f"n{n}_fit"])) < n  # tie-heavy
    for higher_better in (True, False):
        got = C.fused_rank(fit.cuda(), 2, higher_better).cpu()
        want = torch.from_numpy(golden[f"n{n}_hb{int(higher_better)}_out"])
        assert torch.equal(got, want), (n, higher_better, int((got != want).sum()))


# ---------------------------------------------------------------------------
# 2. update against the chain
# ---------------------------------------------------------------------------

UPDATE_BOUND = 65536
UPDATE_LENGTHS = [1, 7, 255, 256, 257, 6409, UPDATE_BOUND, UPDATE_BOUND + 1]
STEP_SIZE, MOMENTUM, SIGMA_LR = 0.1125, 0.9, 0.1
# max_speed below the first step's length (= STEP_SIZE): the clip fires; far
# above anything three steps can reach (< 3 * STEP_SIZE): it never does
SPEEDS = {"clipped": 0.5 * STEP_SIZE, "free": 100.0 * STEP_SIZE}
BOUNDS = {
    "max_change": dict(stdev_min=None, stdev_max=None, stdev_max_change=0.2),
    "max_change+min+max": dict(stdev_min=0.7, stdev_max=1.6, stdev_max_change=0.2),
    "min+max": dict(stdev_min=0.7, stdev_max=1.6, stdev_max_change=None),
    "none": dict(stdev_min=None, stdev_max=None, stdev_max_change=None),
}


def _update_inputs(length):
    g = torch.Generator().manual_seed(length)
    mu = torch.randn(length, generator=g)
    sigma = 0.5 + 1.5 * torch.rand(length, generator=g)
    mu_grads, sigma_grads = [], []
    for step in range(3):
        # step 1 has an all-zero mu gradient (the 1e-30 floor of the norm)
        mu_grads.append(torch.zeros(length) if step == 1 else 3.0 * torch.randn(length, generator=g))
        # by element and step in turn: far below (the relative clamp binds
        # from below), far above (binds from above), small (does not bind)
        kind = (torch.arange(length) + step) % 3
        sg = torch.where(kind == 0, torch.tensor(-10.0), torch.where(kind == 1, torch.tensor(10.0), torch.tensor(0.0)))
        sigma_grads.append(sg + 0.01 * torch.randn(length, generator=g))
    return mu, sigma, mu_grads, sigma_grads


def _chain_update(mu, sigma, velocity, mu_grad, sigma_grad, max_speed, bounds):
    """The launches the fused op replaces: the ops, `+`, and modify_tensor."""
    from evotorch_amd import ops
    from evotorch_amd.utils import modify_tensor

    ops.clipup_step_(velocity, mu_grad, step_size=STEP_SIZE, max_speed=max_speed, momentum=MOMENTUM)
    new_mu = mu + velocity
    target = torch.add(sigma, sigma_grad, alpha=SIGMA_LR)
    if any(v is not None for v in bounds.values()):
        new_sigma = modify_tensor(sigma, target, lb=bounds["stdev_min"], ub=bounds["stdev_max"], max_change=bounds["stdev_max_change"])
    else:
        new_sigma = target
    return new_mu, new_sigma, target


@gpu
@requires_gpu
@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("speed", list(SPEEDS))
@pytest.mark.parametrize("length", UPDATE_LENGTHS)
def test_gaussian_clipup_update_equals_chain(length, speed, bounds_name):
    import evotorch_amd._C as C
    from evotorch_amd import ops

    assert ops.GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH == C.gaussian_clipup_update_max_length() == UPDATE_BOUND
    bounds, max_speed = BOUNDS[bounds_name], SPEEDS[speed]
    mu0, sigma0, mu_grads, sigma_grads = _update_inputs(length)
    mu_f, sigma_f, vel_f = mu0.cuda(), sigma0.cuda(), torch.zeros(length, device="cuda")
    mu_c, sigma_c, vel_c = mu0.cuda(), sigma0.cuda(), torch.zeros(length, device="cuda")
    below = above = inside = False
    for step in range(3):
        mg, sg = mu_grads[step].cuda(), sigma_grads[step].cuda()
        old_sigma = sigma_c
        mu_c, sigma_c, target = _chain_update(mu_c, sigma_c, vel_c, mg, sg, max_speed, bounds)
        # L = bound + 1 goes through the op's own chain and must still agree
        mu_f, sigma_f = ops.gaussian_clipup_update(
            mu_f, sigma_f, vel_f, mg, sg, step_size=STEP_SIZE, max_speed=max_speed, momentum=MOMENTUM, sigma_lr=SIGMA_LR, **bounds
        )
        assert torch.equal(vel_f, vel_c), (step, int((vel_f != vel_c).sum()))
        assert torch.equal(mu_f, mu_c), (step, int((mu_f != mu_c).sum()))
        assert torch.equal(sigma_f, sigma_c), (step, int((sigma_f != sigma_c).sum()))
        assert torch.isfinite(mu_c).all() and torch.isfinite(sigma_c).all()
        speed_now = float(torch.linalg.vector_norm(vel_c.double()))
        if step == 0:
            # the first step alone is STEP_SIZE long
            expected = max_speed if speed == "clipped" else STEP_SIZE
            assert abs(speed_now - expected) < 1e-4 * expected, (speed_now, expected)
        if bounds["stdev_max_change"] is not None:
            # where the relative clamp itself binds (the scalar bounds come on top)
            allowed = old_sigma.abs() * bounds["stdev_max_change"]
            low, high = target < old_sigma - allowed, target > old_sigma + allowed
            below |= bool(low.any())
            above |= bool(high.any())
            inside |= bool((~low & ~high).any())
            if bounds["stdev_min"] is None:
                assert torch.equal(sigma_c[low], (old_sigma - allowed)[low])
                assert torch.equal(sigma_c[high], (allowed + old_sigma)[high])
                assert torch.equal(sigma_c[~low & ~high], target[~low & ~high])
    if bounds["stdev_max_change"] is not None:
        assert below and above and inside, (below, above, inside)


# ---------------------------------------------------------------------------
# 3. obs-norm against the chain
# ---------------------------------------------------------------------------

OBS_DIMS = [1, 17, 376]
COUNTS = [1.0, 4.0e6, float(2**24 + 1), 3.0e9]
MIN_VARIANCE = 1e-2


def _running_sums(obs_dim, count, offset, g):
    """(sum, sumsq) of `count` observations whose columns are, in turn:
    ordinary (variance ~1), nearly constant (variance below min_variance),
    and constant up to rounding with sumsq a shade short, so that
    sumsq / c - mean**2 cancels to a negative number."""
    kind = (torch.arange(obs_dim) + offset) % 3
    mean = 1.0 + torch.rand(obs_dim, generator=g, dtype=torch.float64)
    var = torch.where(kind == 0, 0.5 + torch.rand(obs_dim, generator=g, dtype=torch.float64), torch.tensor(1e-4, dtype=torch.float64))
    total = mean * count
    total_sq = torch.where(kind == 2, mean**2 * count * (1.0 - 1e-5), (mean**2 + var) * count)
    return total.to(torch.float32), total_sq.to(torch.float32)


@gpu
@requires_gpu
@pytest.mark.parametrize("obs_dim", OBS_DIMS)
def test_obsnorm_pack_equals_runningnorm(obs_dim):
    from evotorch_amd import ops
    from evotorch_amd.neuroevolution.runningnorm import RunningNorm
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    spec = SyntheticEnvSpec(obs_dim=obs_dim, act_dim=3, rank=2)
    zeros, ones = torch.zeros(obs_dim, device="cuda"), torch.ones(obs_dim, device="cuda")
    blob = spec.env_blob(zeros, ones, device="cuda").clone()  # persistent: packed in place below
    g = torch.Generator().manual_seed(obs_dim)
    floored = negative = ordinary = False
    for count in COUNTS:
        for offset in range(3):
            rn = RunningNorm(shape=obs_dim, device="cuda", min_variance=MIN_VARIANCE)
            total, total_sq = _running_sums(obs_dim, count, offset, g)
            rn._count.fill_(count)
            rn._sum.copy_(total)
            rn._sum_sq.copy_(total_sq)
            rn._has_data = True
            mean, stdev = rn.mean, rn.stdev
            c = torch.clamp(rn._count, min=1.0).to(torch.float32)
            var = rn._sum_sq / c - mean**2
            floored |= bool(((var < MIN_VARIANCE) & (var >= 0)).any())
            negative |= bool((var < 0).any())
            ordinary |= bool((var > MIN_VARIANCE).any())
            assert ops.obsnorm_pack_(blob, blob.numel() - 2 * obs_dim, rn._count, rn._sum, rn._sum_sq, rn.min_variance)
            # successive different (mean, std) into the same blob: each time
            # the whole blob is the old concatenation
            assert torch.equal(blob[-2 * obs_dim : -obs_dim], mean), (count, offset)
            assert torch.equal(blob[-obs_dim:], stdev), (count, offset)
            assert torch.equal(blob, spec.env_blob(mean, stdev, device="cuda")), (count, offset)
    assert floored and negative and ordinary, (floored, negative, ordinary)


@gpu
@requires_gpu
@pytest.mark.parametrize("c_as", ["float", "tensor32", "tensor64"])
@pytest.mark.parametrize("obs_dim", OBS_DIMS)
def test_obsnorm_merge_equals_update(obs_dim, c_as):
    from evotorch_amd import ops
    from evotorch_amd.neuroevolution.runningnorm import RunningNorm

    g = torch.Generator().manual_seed(100 + obs_dim)
    fused = RunningNorm(shape=obs_dim, device="cuda")
    chain = RunningNorm(shape=obs_dim, device="cuda")
    for count in COUNTS:
        s = (torch.randn(obs_dim, generator=g) * count).to(torch.float32).cuda()
        ss = (torch.rand(obs_dim, generator=g) * count).to(torch.float32).cuda()
        if c_as == "float":
            c = count
        else:
            c = torch.tensor(count, dtype=torch.float32 if c_as == "tensor32" else torch.float64, device="cuda")
        fused.update((c, s, ss))
        with ops.unfused_generation_tail():
            chain.update((c, s, ss))
        assert fused.has_data and chain.has_data
        assert torch.equal(fused._count, chain._count), (count, float(fused._count), float(chain._count))
        assert torch.equal(fused._sum, chain._sum)
        assert torch.equal(fused._sum_sq, chain._sum_sq)
    expected = sum(float(np.float32(c)) if c_as == "tensor32" else c for c in COUNTS)
    assert float(fused._count) == expected


# ---------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------

E2E_CASES = [(18, 0), (18, 64), (32, 0), (32, 64)]


def _pgpe_run(popsize, hidden, generations=5):
    """PGPE + ClipUp, distributed, on the synthetic rollout problem (T = 7):
    what a caller holds after `generations` steps, on the CPU."""
    from evotorch_amd.algorithms import PGPE
    from evotorch_amd.neuroevolution import SyntheticRolloutProblem
    from evotorch_amd.parallel import Comm

    problem = SyntheticRolloutProblem(device="cuda:0", seed=3, episode_length=7, policy_hidden=hidden)
    problem.use_comm(Comm(device=torch.device("cuda", 0)))
    searcher = PGPE(
        problem,
        popsize=popsize,
        radius_init=2.25,
        center_learning_rate=0.1125,
        stdev_learning_rate=0.1,
        optimizer="clipup",
        optimizer_config={"max_speed": 0.15},
        ranking_method="centered",
        distributed=True,
    )
    for _ in range(generations):
        searcher.step()
    status = searcher.status
    count, s, ss = problem.obs_norm.stats_triple()

    def plain(t):
        return torch.Tensor.as_subclass(torch.as_tensor(t).detach(), torch.Tensor).cpu()

    return {
        "center": plain(status["center"]),
        "stdev": plain(status["stdev"]),
        "mean_eval": torch.tensor(float(status["mean_eval"]), dtype=torch.float64),
        "obs_count": plain(count),
        "obs_sum": plain(s),
        "obs_sumsq": plain(ss),
        "fitnesses": plain(problem._grad_batch_cache._evals[:, searcher.obj_index]),
    }


@functools.lru_cache(maxsize=None)
def _fused_run(popsize, hidden):
    """Computed once per case and shared (callers must not modify it)."""
    return _pgpe_run(popsize, hidden)


@gpu
@requires_gpu
@pytest.mark.parametrize("popsize,hidden", E2E_CASES)
def test_fused_tail_equals_unfused(popsize, hidden, monkeypatch):
    from evotorch_amd import ops
    from evotorch_amd.algorithms import gaussian

    fused = _fused_run(popsize, hidden)
    calls = []
    real = ops.gaussian_clipup_update
    monkeypatch.setattr(gaussian.ops, "gaussian_clipup_update", lambda *a, **k: calls.append(1) or real(*a, **k))
    with ops.unfused_generation_tail():
        unfused = _pgpe_run(popsize, hidden)
    assert not calls  # the searcher's own chain ran, not the op
    for name, value in fused.items():
        assert torch.equal(value, unfused[name]), name


@gpu
@requires_gpu
@pytest.mark.parametrize("popsize,hidden", E2E_CASES)
def test_fused_tail_equals_recorded(popsize, hidden):
    """The long vectors (center, stdev) are recorded as the SHA-256 of their
    bytes plus their first 16 elements, everything else in full."""
    import hashlib

    golden = np.load(os.path.join(GOLDEN_DIR, "generation_tail_e2e.npz"))
    for name, value in _fused_run(popsize, hidden).items():
        key = f"p{popsize}_h{hidden}_{name}"
        if key in golden.files:
            assert torch.equal(value, torch.from_numpy(golden[key])), name
            continue
        array = np.ascontiguousarray(value.numpy())
        assert f"{array.dtype}{array.shape}" == str(golden[key + "_dtype_shape"]), name
        assert np.array_equal(array[:16], golden[key + "_head"]), name
        assert hashlib.sha256(array.tobytes()).hexdigest() == str(golden[key + "_sha256"]), name


def _sphere(x):
    return (x**2).sum(-1)


@gpu
@requires_gpu
@pytest.mark.parametrize("config", ["adam", "tensor_max_change"])
def test_configurations_that_fall_back(config, monkeypatch):
    """Adam, or a stdev bound given as a vector, cannot take the one-launch
    update: the searcher's chain runs and follows the CPU trajectory at the
    tolerance of the optimizer-step tests (tests/test_gpu_kernels.py)."""
    from evotorch_amd.algorithms import PGPE, gaussian
    from evotorch_amd.core import Problem

    length = 23

    def forbidden(*args, **kwargs):
        raise AssertionError("the fused update ran for a configuration that must fall back")

    monkeypatch.setattr(gaussian.ops, "gaussian_clipup_update", forbidden)
    g = torch.Generator().manual_seed(5)
    center = torch.randn(length, generator=g)
    grads = [{"mu": torch.randn(length, generator=g), "sigma": 3.0 * torch.randn(length, generator=g)} for _ in range(3)]
    results = {}
    for device in ("cpu", "cuda"):
        problem = Problem("min", _sphere, solution_length=length, initial_bounds=(-1.0, 1.0), device=device, seed=1, vectorized=True)
        if config == "adam":
            kwargs = dict(optimizer="adam", stdev_max_change=0.2)
        else:
            kwargs = dict(optimizer="clipup", stdev_max_change=torch.linspace(0.05, 0.3, length))
        searcher = PGPE(problem, popsize=10, center_init=center, stdev_init=1.0, center_learning_rate=0.1, stdev_learning_rate=0.1, **kwargs)
        for grad in grads:
            searcher._update_distribution({k: v.to(device) for k, v in grad.items()})
        results[device] = (searcher.status["center"], searcher.status["stdev"])
    for on_cpu, on_gpu in zip(results["cpu"], results["cuda"]):
        on_cpu = torch.Tensor.as_subclass(on_cpu, torch.Tensor)
        on_gpu = torch.Tensor.as_subclass(on_gpu, torch.Tensor).cpu()
        assert not torch.equal(on_cpu, center)
        assert torch.allclose(on_gpu, on_cpu, rtol=1e-4, atol=1e-6), (on_gpu - on_cpu).abs().max()
