"""K13 `ops.population_forward` against the vmap path it replaces.

(a) One population forward at n members for the stacks 32 -> 16 -> 8,
376 -> 64 -> 17 (tanh between the layers) and the single layer 376 -> 17,
through `ModuleExpectingFlatParameters`: the kernel, and the vmap path
(`eager_on_gpu()`). Device events, a warm-up of each, the variants
alternating round by round in one process; a sample is --reps forwards
between two events, since one forward is tens of microseconds.

(b) One PGPE generation of `VecEnvNE` on `SyntheticTorchEnv` at popsize n and
T steps, eager and with `use_hip_graph=True`, with the kernel and with the
policy held on the vmap path (what the parent commit runs), for the policy
32 -> 16 -> 8 on a 32/8 environment and for the linear 376 -> 17 policy of
the 81.6 / 37.8 ms row in profiles/general_vs_fused_r2.log.

    python scripts/measure_population_forward.py [--popsize 2048] [--steps 200] [--rounds 10]

Prints one JSON line per stack and per generation setup. Run it twice.
"""

import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(run):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    run()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def _alternate(variants, rounds, warmup, reps=1):
    """mean/stdev/min/max of a call's time in ms; a sample is `reps` calls between two events."""
    for run in variants.values():
        for _ in range(warmup):
            run()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, run in variants.items():
            times[name].append(_timed(lambda: [run() for _ in range(reps)]) / reps)
    return {
        name: {"mean_ms": statistics.mean(ts), "stdev_ms": statistics.stdev(ts), "min_ms": min(ts), "max_ms": max(ts)}
        for name, ts in times.items()
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="forwards per timed sample in (a)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"

    from evotorch_amd import ops
    from evotorch_amd.algorithms import PGPE
    from evotorch_amd.models.functional import make_functional_module
    from evotorch_amd.neuroevolution import SyntheticTorchEnv, VecEnvNE

    n, T = args.popsize, args.steps
    g = torch.Generator().manual_seed(0)
    stacks = {
        "32-16-8": nn.Sequential(nn.Linear(32, 16), nn.Tanh(), nn.Linear(16, 8)),
        "376-64-17": nn.Sequential(nn.Linear(376, 64), nn.Tanh(), nn.Linear(64, 17)),
        "376-17": nn.Linear(376, 17),
    }
    for name, net in stacks.items():
        fmodule = make_functional_module(net)
        assert fmodule._dense_stack is not None
        d0 = fmodule._dense_stack[0][0]
        params = (0.1 * torch.randn(n, fmodule.parameter_count, generator=g)).cuda()
        obs = torch.randn(n, d0, generator=g).cuda()

        def vmapped():
            with ops.eager_on_gpu():
                return fmodule(params, obs)

        variants = {"kernel": lambda: fmodule(params, obs), "vmap": vmapped}
        max_diff = (variants["kernel"]() - variants["vmap"]()).abs().max().item()
        rows = _alternate(variants, args.rounds, args.warmup, args.reps)
        print(json.dumps({"forward": name, "n": n, "rounds": args.rounds, "reps": args.reps, "max_abs_diff": max_diff,
                          "vmap_over_kernel": rows["vmap"]["mean_ms"] / rows["kernel"]["mean_ms"], "variants": rows}),
              flush=True)

    setups = {
        "32-16-8": ("Linear(obs_length, 16) >> Tanh() >> Linear(16, act_length)", dict(obs_dim=32, act_dim=8, rank=8)),
        "376-17": ("Linear(obs_length, act_length)", {}),
    }
    for name, (net, env_kwargs) in setups.items():
        searchers = {}
        for graphed in (False, True):
            for kernel in (True, False):
                prob = VecEnvNE(
                    lambda k: SyntheticTorchEnv(num_envs=k, episode_length=T, device="cuda:0", **env_kwargs),
                    net, device="cuda:0", seed=1, max_num_steps=T, use_hip_graph=graphed,
                )
                if not kernel:  # hold this problem's policy on the vmap path, as before K13
                    prob._policy = prob.make_functional_policy()
                    prob._policy._fmodule._dense_stack = None
                r = 2.25
                searcher = PGPE(prob, popsize=n, radius_init=r, center_learning_rate=0.75 * r / 15,
                                stdev_learning_rate=0.1, optimizer="clipup", optimizer_config={"max_speed": r / 15},
                                distributed=True)
                searchers[("graphed" if graphed else "eager") + ("_kernel" if kernel else "_vmap")] = searcher.step
        rows = _alternate(searchers, args.rounds, args.warmup)
        print(json.dumps({"generation": name, "popsize": n, "steps": T, "rounds": args.rounds, "variants": rows}),
              flush=True)


if __name__ == "__main__":
    main()
