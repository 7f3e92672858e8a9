"""Five PGPE generations on `SyntheticRolloutProblem` at popsize 64, T = 3,
with the fused generation tail (where `mean_eval` is one launch of
`_C.nanmean_1d`) against the same run under `ops.unfused_generation_tail()`
(where it is `torch.nanmean`): every generation's `center`, `stdev`,
`mean_eval` and fitness vector equal (`torch.equal`), with and without
`store_solution_stats`.

The comparison is of two paths, not of one with itself: `_C.nanmean_1d` is
called exactly once per generation, on the generation's fitness vector, with
the fused tail on, and never under `unfused_generation_tail()`.
"""

import functools

import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

POPSIZE, STEPS, GENERATIONS = 64, 3, 5


def _plain(t):
    return torch.Tensor.as_subclass(torch.as_tensor(t).detach(), torch.Tensor).cpu().clone()


def _run(store_solution_stats):
    """(what a caller sees after each generation, the lengths `_C.nanmean_1d`
    was called with in each generation)."""
    import evotorch_amd._C as C
    from evotorch_amd.algorithms import PGPE
    from evotorch_amd.neuroevolution import SyntheticRolloutProblem
    from evotorch_amd.parallel import Comm

    calls = []
    real = C.nanmean_1d

    def spy(x):
        calls.append((x.numel(), x.data_ptr()))
        return real(x)

    C.nanmean_1d = spy
    try:
        problem = SyntheticRolloutProblem(device="cuda:0", seed=23, episode_length=STEPS, observation_normalization=True)
        problem._store_solution_stats = bool(store_solution_stats)
        problem.use_comm(Comm(device=torch.device("cuda", 0)))
        searcher = PGPE(
            problem,
            popsize=POPSIZE,
            radius_init=2.25,
            center_learning_rate=0.1125,
            stdev_learning_rate=0.1,
            optimizer="clipup",
            optimizer_config={"max_speed": 0.15},
            ranking_method="centered",
            distributed=True,
        )
        history, calls_per_generation = [], []
        for _ in range(GENERATIONS):
            before = len(calls)
            searcher.step()
            mean_eval = searcher.status["mean_eval"]
            fitnesses = _plain(problem._grad_batch_cache.evals[:, 0])
            calls_per_generation.append([n for n, _ in calls[before:]])
            history.append(
                {
                    "center": _plain(searcher.status["center"]),
                    "stdev": _plain(searcher.status["stdev"]),
                    "mean_eval": torch.tensor(float(mean_eval), dtype=torch.float64),
                    "fitnesses": fitnesses,
                }
            )
    finally:
        C.nanmean_1d = real
    return history, calls_per_generation


@functools.lru_cache(maxsize=None)
def _runs(store_solution_stats):
    """(fused, unfused), computed once per case and shared read-only."""
    from evotorch_amd import ops

    fused = _run(store_solution_stats)
    with ops.unfused_generation_tail():
        unfused = _run(store_solution_stats)
    return fused, unfused


@gpu
@requires_gpu
@pytest.mark.parametrize("store_solution_stats", [False, True], ids=["plain", "solution_stats"])
def test_fused_tail_equals_unfused_every_generation(store_solution_stats):
    (fused, _), (unfused, _) = _runs(store_solution_stats)
    assert len(fused) == len(unfused) == GENERATIONS
    for g, (a, b) in enumerate(zip(fused, unfused)):
        assert a.keys() == b.keys() == {"center", "stdev", "mean_eval", "fitnesses"}
        for name in a:
            assert torch.equal(a[name], b[name]), (g, name)
        assert a["fitnesses"].shape == (POPSIZE,) and bool(torch.isfinite(a["fitnesses"]).all())
        # mean_eval is the mean of THIS generation's fitnesses. An fp32 sum of
        # n terms in any order is within (n - 1)·u·Σ|x| of the exact one
        # (u = 2^-24), the division adds one rounding of the mean.
        f64 = a["fitnesses"].double()
        bound = POPSIZE * 2.0**-24 * float(f64.abs().mean()) + 2.0**-23 * abs(float(f64.mean()))
        assert abs(float(a["mean_eval"]) - float(f64.mean())) <= bound, g
    assert not torch.equal(fused[0]["center"], fused[-1]["center"])
    assert not torch.equal(fused[0]["mean_eval"], fused[-1]["mean_eval"])


@gpu
@requires_gpu
@pytest.mark.parametrize("store_solution_stats", [False, True], ids=["plain", "solution_stats"])
def test_mean_eval_takes_the_kernel_once_per_generation(store_solution_stats):
    (_, fused_calls), (_, unfused_calls) = _runs(store_solution_stats)
    assert fused_calls == [[POPSIZE]] * GENERATIONS
    assert unfused_calls == [[]] * GENERATIONS
