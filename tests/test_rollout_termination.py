"""Early episode termination in the fused rollout: `SyntheticEnvSpec(healthy_range=...)`,
`rollout_eager`, `SyntheticTorchEnv`, `SyntheticRolloutProblem` and the
terminating v6 kernel `_C.rollout_terminating`.

Shared inputs: the eight geometries, NS, `_norm`, `_params` and SEED of
tests/test_gpu_rollout_general.py (copied, not imported), 8-step episodes,
health_index 0 and healthy_range (-Z, Z) with one Z for every case.

Z = 0.3325. Over all 24 (case, n) pairs the smallest distance of a counted
|bf16(o'[0])| from Z is printed by `TestInputs.test_margin_and_spread`
(0.0102 when Z was chosen) and must be at least 4 * 2**-9: bf16 values
below 0.5 are at most 2**-9 apart, so a kernel whose o'[0] rounds one bf16
step away from the reference's cannot flip a termination, and the GPU
tests demand exact lengths from every member.
"""

import functools
import math

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

# tolerances of TestRollout.test_matches_eager_reference
FIT_TOL = dict(rtol=2e-2, atol=2e-2)
STAT_TOL = dict(rtol=5e-2, atol=5e-1)
SEED = 41
STEPS = 8
Z = 0.3325
MIN_MARGIN = 4 * 2.0**-9

# (obs_dim, act_dim, rank, policy_hidden, force_v6): see tests/test_gpu_rollout_general.py
CASES = {
    "linear_base": (32, 8, 8, 0, False),
    "linear_odd": (20, 3, 5, 0, False),
    "mlp_tail_only": (20, 3, 5, 6, False),
    "mlp_base": (32, 8, 8, 16, False),
    "wide_obs": (300, 4, 4, 0, False),
    "one_member": (376, 17, 16, 96, False),
    "humanoid_linear_v6": (376, 17, 16, 0, True),
    "humanoid_mlp64_v6": (376, 17, 16, 64, True),
}
NS = (1, 2, 5)


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


def _spec(case, healthy_range=(-Z, Z), steps=STEPS):
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    O, A, R, H, _ = CASES[case]
    return SyntheticEnvSpec(
        episode_length=steps, obs_dim=O, act_dim=A, rank=R, policy_hidden=H, healthy_range=healthy_range
    )


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
def _reference(case, n, terminating=True, steps=STEPS):
    """CPU reference (fitness, sum, sumsq, count, lengths), computed once per
    key and shared: callers must not modify it."""
    from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

    spec = _spec(case, (-Z, Z) if terminating else None, steps)
    mean, std = _norm(spec.obs_dim)
    fit, (count, s, sq), lengths = rollout_eager(spec, _params(case, n), mean, std, init_seed=SEED, return_steps=True)
    assert torch.isfinite(fit).all() and torch.isfinite(s).all() and torch.isfinite(sq).all()
    return fit, s, sq, count, lengths


@functools.lru_cache(maxsize=None)
def _health_trace(case, n):
    """Step-by-step replay of the fixed-length episode, written out here from
    the environment's definition: the bf16 o'[0] after every step, [STEPS, n],
    and the fitness after every step, [STEPS, n]."""
    spec = _spec(case, None)
    O, A, H = spec.obs_dim, spec.act_dim, spec.policy_hidden
    params = _params(case, n)
    mean, std = _norm(O)

    def q(x):
        return x.to(torch.bfloat16).to(torch.float32)

    if H > 0:
        W1 = q(params[:, : H * O].reshape(n, H, O))
        b1 = params[:, H * O : H * O + H]
        W2 = q(params[:, H * O + H : H * O + H + A * H].reshape(n, A, H))
        b = params[:, H * O + H + A * H :]
    else:
        W = q(params[:, : A * O].reshape(n, A, O))
        b = params[:, A * O :]
    V, U_T, D2_T = q(spec.V), q(spec.U_T), q(spec.D2_T)
    inv_std = 1.0 / std
    obs = q(spec.initial_obs(n, 0, SEED))
    fitness = torch.zeros(n)
    health, fits = [], []
    for _ in range(STEPS):
        obs_n = q((obs - mean) * inv_std)
        if H > 0:
            hid = q(torch.tanh(torch.einsum("nho,no->nh", W1, obs_n) + b1))
            act = torch.clamp(torch.einsum("nah,nh->na", W2, hid) + b, -1.0, 1.0)
        else:
            act = torch.clamp(torch.einsum("nao,no->na", W, obs_n) + b, -1.0, 1.0)
        h = q(obs @ V.T)
        o_new = torch.tanh(h @ U_T + q(act) @ D2_T + spec.c)
        fitness = fitness + o_new @ spec.wr + spec.alive_bonus - spec.act_cost * (act**2).sum(-1) / A
        obs = q(o_new)
        health.append(obs[:, 0].clone())
        fits.append(fitness.clone())
    return torch.stack(health), torch.stack(fits)


def _first_unhealthy(case, n):
    """Episode lengths read from the replay: the first step whose bf16 o'[0]
    is outside (-Z, Z), else STEPS."""
    health, _ = _health_trace(case, n)
    lengths = []
    for m in range(n):
        bad = [t for t in range(STEPS) if not (-Z <= health[t, m].item() <= Z)]
        lengths.append(bad[0] + 1 if bad else STEPS)
    return torch.tensor(lengths, dtype=torch.int64)


ALL_PAIRS = [(case, n) for case in CASES for n in NS]


class TestInputs:
    def test_replay_is_the_reference(self):
        # the replay above and rollout_eager are the same arithmetic
        from evotorch_amd.neuroevolution.synthetic_env import rollout_eager

        for case, n in ALL_PAIRS:
            spec = _spec(case, None)
            mean, std = _norm(spec.obs_dim)
            fit, _ = rollout_eager(spec, _params(case, n), mean, std, init_seed=SEED)
            assert torch.equal(fit, _health_trace(case, n)[1][-1]), case

    def test_margin_and_spread(self):
        margin = math.inf
        split_block = False
        for case, n in ALL_PAIRS:
            lengths = _reference(case, n)[4]
            health, _ = _health_trace(case, n)
            for m in range(n):
                counted = health[: int(lengths[m]), m]
                margin = min(margin, (counted.abs() - Z).abs().min().item())
            print(f"{case} n={n}: lengths={lengths.tolist()}")
            if n == 5:
                # (b) the members are told apart and somebody stops early
                assert len(set(lengths.tolist())) >= 2, (case, lengths)
                assert int(lengths.min()) < STEPS, (case, lengths)
                # (c) a two-member block (all but one_member) whose members die at different steps
                if case != "one_member":
                    for first in (0, 2):
                        pair = lengths[first : first + 2].tolist()
                        if pair[0] != pair[1] and min(pair) < STEPS:
                            split_block = True
        print(f"smallest margin of a counted |bf16(o'[0])| to Z={Z}: {margin:.6f}")
        assert margin >= MIN_MARGIN, margin  # (a)
        assert split_block


class TestSpec:
    def test_defaults(self):
        from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec, rollout_eager

        spec = SyntheticEnvSpec(obs_dim=20, act_dim=3, rank=5, episode_length=STEPS)
        assert spec.healthy_range is None and spec.health_index == 0 and spec.terminates is False
        assert _spec("linear_odd").terminates is True
        mean, std = _norm(20)
        params = _params("linear_odd", 5)
        plain = rollout_eager(spec, params, mean, std, init_seed=SEED)
        assert len(plain) == 2
        for healthy_range in (None, (-math.inf, math.inf)):
            other = rollout_eager(_spec("linear_odd", healthy_range), params, mean, std, init_seed=SEED)
            assert len(other) == 2
            assert torch.equal(other[0], plain[0])
            assert other[1][0] == plain[1][0] == 5.0 * STEPS
            assert torch.equal(other[1][1], plain[1][1]) and torch.equal(other[1][2], plain[1][2])
        with_steps = rollout_eager(spec, params, mean, std, init_seed=SEED, return_steps=True)
        assert len(with_steps) == 3 and with_steps[2].dtype == torch.int64
        assert with_steps[2].tolist() == [STEPS] * 5

    @pytest.mark.parametrize(
        "kwargs",
        [
            dict(healthy_range=(0.5, -0.5)),
            dict(healthy_range=(math.nan, 1.0)),
            dict(healthy_range=(-1.0, math.nan)),
            dict(healthy_range=(-1.0, 1.0), health_index=20),
            dict(health_index=-1),
        ],
    )
    def test_invalid_arguments(self, kwargs):
        from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

        with pytest.raises(ValueError):
            SyntheticEnvSpec(obs_dim=20, act_dim=3, rank=5, **kwargs)

    def test_infinite_bounds_accepted(self):
        from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

        spec = SyntheticEnvSpec(obs_dim=20, act_dim=3, rank=5, healthy_range=(-math.inf, 0.4), health_index=19)
        assert spec.terminates and spec.healthy_range == (-math.inf, 0.4)


class TestEagerTermination:
    @pytest.mark.parametrize("case,n", ALL_PAIRS)
    def test_truncation_identity(self, case, n):
        fit, _, _, count, lengths = _reference(case, n)
        assert lengths.dtype == torch.int64
        assert torch.equal(lengths, _first_unhealthy(case, n))
        assert count == float(lengths.sum())
        for s in sorted(set(lengths.tolist())):
            fixed = _reference(case, n, False, s)[0]
            mask = lengths == s
            assert torch.equal(fit[mask], fixed[mask]), (case, s)

    def test_statistics_count_only_live_steps(self):
        # one member: the sums are those of a fixed-length run of its length
        case = "linear_base"
        _, s, sq, _, lengths = _reference(case, 1)
        assert int(lengths[0]) < STEPS
        _, fs, fsq, fcount, _ = _reference(case, 1, False, int(lengths[0]))
        assert torch.equal(s, fs) and torch.equal(sq, fsq) and fcount == float(lengths[0])


class TestTorchEnv:
    def test_done_at_first_unhealthy_step(self):
        from evotorch_amd.neuroevolution import SyntheticTorchEnv

        n = 5
        env = SyntheticTorchEnv(_spec("linear_base"), num_envs=n)
        free = SyntheticTorchEnv(_spec("linear_base", None), num_envs=n)
        env.reset(seed=SEED)
        free.reset(seed=SEED)
        g = torch.Generator().manual_seed(3)
        seen_early = False
        for t in range(STEPS):
            actions = torch.randn(n, 8, generator=g)
            obs, reward, done = env.step(actions)
            fobs, freward, fdone = free.step(actions)
            assert torch.equal(obs, fobs) and torch.equal(reward, freward)
            unhealthy = ~((obs[:, 0] >= -Z) & (obs[:, 0] <= Z))
            last = t == STEPS - 1
            assert torch.equal(done, unhealthy | last)
            assert torch.equal(fdone, torch.full((n,), last))
            seen_early = seen_early or bool((done & ~fdone).any())
        assert seen_early


def _problem(device, healthy_range=(-Z, Z), **kwargs):
    from evotorch_amd.neuroevolution import SyntheticRolloutProblem

    O, A, R, H, _ = CASES["linear_base"]
    return SyntheticRolloutProblem(
        device=device, seed=5, obs_dim=O, act_dim=A, rank=R, policy_hidden=H, episode_length=STEPS,
        healthy_range=healthy_range, **kwargs,
    )


def _evaluate(problem, n=5):
    from evotorch_amd.core import SolutionBatch

    batch = SolutionBatch(problem, popsize=n, empty=True)
    batch.set_values(_params("linear_base", n).to(problem.device))
    problem.evaluate(batch)
    return batch


class TestProblemCPU:
    def test_lengths_counts_and_rewards(self):
        problem = _problem("cpu")
        assert problem.last_episode_lengths is None
        batch = _evaluate(problem)
        lengths = problem.last_episode_lengths
        assert lengths.dtype == torch.int32 and lengths.shape == (5,)
        assert int(lengths.min()) < STEPS and len(set(lengths.tolist())) >= 2
        total = int(lengths.sum())
        assert problem.last_eval_interaction_count == total
        assert problem.total_interaction_count == total
        assert problem.status["total_interaction_count"] == total
        assert problem.obs_norm.count == float(total)
        _evaluate(problem)
        assert problem.total_interaction_count == total + int(problem.last_episode_lengths.sum())

        d = 0.75
        decreased = _problem("cpu", decrease_rewards_by=d)
        dbatch = _evaluate(decreased)
        assert torch.equal(decreased.last_episode_lengths, lengths)
        expected = batch.evals[:, 0] - d * lengths.to(torch.float32)
        assert torch.allclose(dbatch.evals[:, 0], expected, rtol=0, atol=1e-5)

    def test_fixed_length_problem_is_unchanged(self):
        problem = _problem("cpu", None, decrease_rewards_by=0.5)
        plain = _problem("cpu", None)
        batch, pbatch = _evaluate(problem), _evaluate(plain)
        assert problem.last_eval_interaction_count == 5 * STEPS
        assert isinstance(problem.status["total_interaction_count"], int)
        assert problem.last_episode_lengths.tolist() == [STEPS] * 5
        assert problem.last_episode_lengths.dtype == torch.int32
        assert torch.allclose(batch.evals[:, 0], pbatch.evals[:, 0] - 0.5 * STEPS, rtol=0, atol=1e-5)

    def test_adaptive_popsize(self):
        from evotorch_amd.algorithms import PGPE

        def population(healthy_range):
            problem = _problem("cpu", healthy_range)
            searcher = PGPE(
                problem, popsize=8, num_interactions=8 * STEPS, popsize_max=64,
                center_learning_rate=0.1, stdev_learning_rate=0.1, stdev_init=0.1,
            )
            searcher.step()
            return len(searcher.population)

        assert population(None) == 8
        # most episodes end within a step or two under this range
        grown = population((-0.05, 0.05))
        assert 8 < grown <= 64


# --------------------------------------------------------------------------- GPU


def _run_linear(C, case, n, steps=STEPS):
    spec = _spec(case, None)
    O = spec.obs_dim
    mean, std = _norm(O)
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.zeros(2 * O, device="cuda")
    fit = C.rollout_linear(_params(case, n).cuda().contiguous(), blob, stats, O, spec.act_dim, spec.rank,
                           steps, spec.alive_bonus, spec.act_cost, SEED, 0, spec.policy_hidden)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu()


def _run_terminating(C, case, n, lo=-Z, hi=Z):
    spec = _spec(case, None)
    O = spec.obs_dim
    mean, std = _norm(O)
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.zeros(2 * O, device="cuda")
    lengths = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    fit = C.rollout_terminating(_params(case, n).cuda().contiguous(), blob, stats, lengths, O, spec.act_dim,
                                spec.rank, STEPS, spec.alive_bonus, spec.act_cost, SEED, 0, spec.policy_hidden,
                                0, lo, hi)
    return fit.cpu(), stats[:O].cpu(), stats[O:].cpu(), lengths.cpu()


@pytest.fixture
def kernel_env(monkeypatch):
    def select(case):
        if CASES[case][4]:
            monkeypatch.setenv("EVOTORCH_AMD_ROLLOUT_V6", "1")
        else:
            monkeypatch.delenv("EVOTORCH_AMD_ROLLOUT_V6", raising=False)

    return select


def _deviation(got, want):
    return {key: (g - w).abs().max().item() for key, g, w in zip(("fitness", "sum", "sumsq"), got, want)}


@pytest.fixture(scope="module")
def fixed_length_deviation(C):
    """max |rollout_linear - rollout_eager| of the unchanged fixed-length pair
    at 8 steps, over every case and n (v6 at the Humanoid geometry)."""
    import os

    worst = {"fitness": 0.0, "sum": 0.0, "sumsq": 0.0}
    saved = os.environ.get("EVOTORCH_AMD_ROLLOUT_V6")
    try:
        for case, n in ALL_PAIRS:
            if CASES[case][4]:
                os.environ["EVOTORCH_AMD_ROLLOUT_V6"] = "1"
            else:
                os.environ.pop("EVOTORCH_AMD_ROLLOUT_V6", None)
            dev = _deviation(_run_linear(C, case, n), _reference(case, n, False)[:3])
            for key in worst:
                worst[key] = max(worst[key], dev[key])
    finally:
        if saved is None:
            os.environ.pop("EVOTORCH_AMD_ROLLOUT_V6", None)
        else:
            os.environ["EVOTORCH_AMD_ROLLOUT_V6"] = saved
    print(f"fixed-length kernel vs eager at {STEPS} steps, all cases: {worst}")
    return worst


@requires_gpu
@pytest.mark.gpu
class TestTerminatingKernel:
    @pytest.mark.parametrize("case,n", ALL_PAIRS)
    def test_never_terminating_equals_fixed_length(self, C, kernel_env, case, n):
        kernel_env(case)
        fit, s, sq, lengths = _run_terminating(C, case, n, -math.inf, math.inf)
        lfit, ls, lsq = _run_linear(C, case, n)
        assert lengths.tolist() == [STEPS] * n
        assert torch.equal(fit, lfit)
        assert torch.equal(s, ls) and torch.equal(sq, lsq)

    @pytest.mark.parametrize("case,n", ALL_PAIRS)
    def test_lengths_and_truncation_identity(self, C, kernel_env, case, n):
        kernel_env(case)
        fit, _, _, lengths = _run_terminating(C, case, n)
        assert lengths.dtype == torch.int32
        assert lengths.tolist() == _reference(case, n)[4].tolist()
        for s in sorted(set(lengths.tolist())):
            fixed = _run_linear(C, case, n, steps=s)[0]
            mask = lengths == s
            assert torch.equal(fit[mask], fixed[mask]), (case, s, fit, fixed)

    @pytest.mark.parametrize("case,n", ALL_PAIRS)
    def test_matches_eager(self, C, fixed_length_deviation, case, n):
        fit, s, sq, _ = _run_terminating(C, case, n)
        efit, es, esq = _reference(case, n)[:3]
        dev = _deviation((fit, s, sq), (efit, es, esq))
        print(f"{case} n={n}: terminating max|dfit|={dev['fitness']:.4e} max|dsum|={dev['sum']:.4e} "
              f"max|dsumsq|={dev['sumsq']:.4e}; fixed-length, all cases: {fixed_length_deviation}")
        for key, d in dev.items():
            assert d <= 2 * fixed_length_deviation[key], (key, d)
        assert torch.allclose(fit, efit, **FIT_TOL), (fit, efit)
        assert torch.allclose(s, es, **STAT_TOL)
        assert torch.allclose(sq, esq, **STAT_TOL)

    def test_bitwise_repeatable(self, C):
        a = _run_terminating(C, "wide_obs", 5)
        b = _run_terminating(C, "wide_obs", 5)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# Operand checks in the style of tests/test_gpu_kernel_args.py. A bad
# steps_out is longer than the kernel writes or of a wider dtype; the
# host-resident one is stopped by the device check every operand gets first.
SENTINEL = -7
O1, A1, R1 = 32, 8, 8


def _terminating_call(C, steps_out, health_index=0, lo=-Z, hi=Z, n=2):
    spec = _spec("linear_base", None)
    mean, std = _norm(O1)
    blob = spec.env_blob(mean.cuda(), std.cuda(), device="cuda")
    stats = torch.full((2 * O1,), float(SENTINEL), device="cuda")
    params = _params("linear_base", n).cuda().contiguous()
    try:
        fit = C.rollout_terminating(params, blob, stats, steps_out, O1, A1, R1, STEPS, spec.alive_bonus,
                                    spec.act_cost, SEED, 0, 0, health_index, lo, hi)
    except RuntimeError:
        assert bool((stats == SENTINEL).all()) and bool((steps_out == SENTINEL).all())  # nothing was touched
        raise
    return fit, stats


def _steps_out(n=2, dtype=torch.int32, device="cuda"):
    return torch.full((n,), SENTINEL, dtype=dtype, device=device)


REJECTED = {
    "steps_out_cpu": ("steps_out", lambda: dict(steps_out=_steps_out(device="cpu"))),
    "steps_out_int64": ("steps_out", lambda: dict(steps_out=_steps_out(dtype=torch.int64))),
    "steps_out_long": ("steps_out", lambda: dict(steps_out=_steps_out(n=4))),
    "health_index_O": ("health_index", lambda: dict(steps_out=_steps_out(), health_index=O1)),
    "lo_above_hi": ("lo <= hi", lambda: dict(steps_out=_steps_out(), lo=0.5, hi=-0.5)),
    "nan_bound": ("lo <= hi", lambda: dict(steps_out=_steps_out(), lo=math.nan, hi=0.5)),
}


@requires_gpu
@pytest.mark.gpu
class TestTerminatingOperands:
    @pytest.mark.parametrize("name", list(REJECTED))
    def test_rejected(self, C, name):
        phrase, kwargs = REJECTED[name]
        with pytest.raises(RuntimeError, match=phrase):
            _terminating_call(C, **kwargs())

    @pytest.mark.parametrize("kwargs", [dict(), dict(health_index=O1 - 1), dict(lo=0.25, hi=0.25)])
    def test_accepted(self, C, kwargs):
        steps_out = _steps_out()
        fit, stats = _terminating_call(C, steps_out, **kwargs)
        assert torch.isfinite(fit).all() and torch.isfinite(stats).all()
        assert bool(((steps_out >= 1) & (steps_out <= STEPS)).all())
        if not kwargs:
            assert steps_out.tolist() == _reference("linear_base", 2)[4].tolist()


@requires_gpu
@pytest.mark.gpu
class TestProblemGPU:
    def test_matches_cpu_problem(self, monkeypatch):
        # a CPU and a ROCm generator derive different episode seeds from the
        # same problem seed: pin the episode seed itself
        import evotorch_amd.neuroevolution.synthetic as synthetic

        monkeypatch.setattr(synthetic, "seed_from_generator", lambda generator, device: SEED)
        gpu, cpu = _problem("cuda:0"), _problem("cpu")
        assert gpu.last_episode_lengths is None
        gbatch, cbatch = _evaluate(gpu), _evaluate(cpu)
        lengths = gpu.last_episode_lengths
        assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.shape == (5,)
        assert torch.equal(lengths.cpu(), cpu.last_episode_lengths)
        assert torch.allclose(gbatch.evals[:, 0].cpu(), cbatch.evals[:, 0], **FIT_TOL)
        total = int(lengths.sum())
        assert gpu.obs_norm.count == float(total)
        assert gpu.last_eval_interaction_count == total
        assert gpu.total_interaction_count == total
        assert int(gpu.status["total_interaction_count"]) == total

    def test_decrease_rewards_by(self):
        plain, decreased = _problem("cuda:0"), _problem("cuda:0", decrease_rewards_by=0.75)
        pbatch, dbatch = _evaluate(plain), _evaluate(decreased)
        lengths = plain.last_episode_lengths
        assert torch.equal(lengths, decreased.last_episode_lengths)
        expected = pbatch.evals[:, 0] - 0.75 * lengths.to(torch.float32)
        assert torch.allclose(dbatch.evals[:, 0], expected, rtol=0, atol=1e-5)

    def test_graph_capture_keeps_counting(self):
        from evotorch_amd.algorithms import PGPE, GraphedSearch

        problem = _problem("cuda:0", (-0.2, 0.2))
        searcher = PGPE(
            problem, popsize=16, center_learning_rate=0.1, stdev_learning_rate=0.1, stdev_init=0.1,
            optimizer="clipup", optimizer_config=dict(max_speed=0.2),
        )
        graphed = GraphedSearch(searcher).capture()
        before = problem.total_interaction_count
        counted = 0
        seen = []
        for _ in range(3):
            graphed.run(1)
            lengths = problem.last_episode_lengths
            assert lengths.shape == (16,)
            seen.append(lengths.tolist())
            assert problem.last_eval_interaction_count == int(lengths.sum())
            counted += int(lengths.sum())
        assert problem.total_interaction_count - before == counted
        assert 16 <= min(sum(s) for s in seen) and max(sum(s) for s in seen) < 16 * STEPS
