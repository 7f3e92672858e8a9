"""Cost and gain of early termination in the rollout kernels.

At the Humanoid geometry (obs 376, act 17, rank 16), for the linear and the
MLP-64 policy, one process times these launches with device events, after a
warm-up of each, alternating them round by round:

  v6_fixed     `rollout_linear` forced to the general kernel
  v6_term_inf  `rollout_terminating` forced to v6, range (-inf, inf): same work
  v6_term_z    `rollout_terminating` forced to v6, range (-z, z), for every --z
  v7_or_m7     `rollout_linear` as dispatched by default (v7 linear, m7 MLP-64)
  v7_term_inf  `rollout_terminating` as dispatched by default, range (-inf, inf)
  v7_term_z    ... and range (-z, z), for every --z        (linear policy only)

The v6 rows set EVOTORCH_AMD_ROLLOUT_V6, the others clear it, and every row
asserts through `_C.rollout_kernel_name` that it runs the kernel it says.

(a) is v6_term_inf against v6_fixed, beside the spread of each; (b) is
v6_term_z against v6_fixed, beside mean(block-maximum length) / T, the
share of the steps a block cannot skip (2-member blocks); (c) is the
v7_or_m7 row. For the linear policy, v7_term_inf against v7_or_m7 is the
overhead of termination inside v7, and v7_term_z against v6_term_z its gain
over the general kernel, beside the 16-member block maximum.

    python scripts/measure_terminating_rollout.py [--popsize 4000] [--steps 1000] [--rounds 10] [--z 0.8 0.9]

Prints one JSON line per policy.
"""

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

O, A, R = 376, 17, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--z", type=float, nargs="+", default=[0.8, 0.9])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"

    import evotorch_amd._C as C
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    n, T = args.popsize, args.steps
    for H in (0, 64):
        spec = SyntheticEnvSpec(episode_length=T, policy_hidden=H)
        g = torch.Generator().manual_seed(0)
        params = (0.1 * torch.randn(n, spec.solution_length, generator=g)).cuda().contiguous()
        blob = spec.env_blob(torch.zeros(O), torch.ones(O), device="cuda")
        stats = torch.zeros(2 * O, device="cuda")
        lengths = torch.zeros(n, dtype=torch.int32, device="cuda")

        def select(force_v6, terminating, expected):
            if force_v6:
                os.environ["EVOTORCH_AMD_ROLLOUT_V6"] = "1"
            else:
                os.environ.pop("EVOTORCH_AMD_ROLLOUT_V6", None)
            name = C.rollout_kernel_name(O, A, R, H, terminating)
            assert name == expected, (name, expected)

        def fixed(force_v6, expected):
            def run():
                select(force_v6, False, expected)
                return C.rollout_linear(params, blob, stats, O, A, R, T, spec.alive_bonus, spec.act_cost, 3, 0, H)

            return run

        def terminating(force_v6, expected, lo, hi):
            def run():
                select(force_v6, True, expected)
                return C.rollout_terminating(
                    params, blob, stats, lengths, O, A, R, T, spec.alive_bonus, spec.act_cost, 3, 0, H, 0, lo, hi
                )

            return run

        variants = {"v6_fixed": fixed(True, "v6"), "v6_term_inf": terminating(True, "v6", -math.inf, math.inf)}
        for z in args.z:
            variants[f"v6_term_z{z}"] = terminating(True, "v6", -z, z)
        variants["v7_or_m7"] = fixed(False, "v7" if H == 0 else "m7")
        if H == 0:
            variants["v7_term_inf"] = terminating(False, "v7", -math.inf, math.inf)
            for z in args.z:
                variants[f"v7_term_z{z}"] = terminating(False, "v7", -z, z)

        episode = {}
        for name, run in variants.items():
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            if "_term" in name:
                len_f = lengths.to(torch.float32).cpu()
                # members of a block: v6 fits two at this geometry for both policies, v7 has 16
                members = 16 if name.startswith("v7") else 2
                padded = torch.cat([len_f, torch.zeros(-n % members)])
                block_max = padded.reshape(-1, members).max(1).values
                episode[name] = {
                    "mean_length": len_f.mean().item(),
                    "block_members": members,
                    "mean_block_max_length": block_max.mean().item(),
                    "block_max_over_T": block_max.mean().item() / T,
                }
        # the never-terminating runs must equal the fixed-length ones bit for bit
        same = torch.equal(variants["v6_fixed"](), variants["v6_term_inf"]())
        if H == 0:
            same = same and torch.equal(variants["v7_or_m7"](), variants["v7_term_inf"]())

        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, run in variants.items():
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                run()
                end.record()
                end.synchronize()
                times[name].append(start.elapsed_time(end))
        os.environ.pop("EVOTORCH_AMD_ROLLOUT_V6", None)

        base = statistics.mean(times["v6_fixed"])
        result = {"policy": "linear" if H == 0 else f"mlp{H}", "popsize": n, "steps": T, "rounds": args.rounds,
                  "term_inf_equals_fixed": same, "variants": {}}
        for name, ts in times.items():
            row = {"mean_ms": statistics.mean(ts), "stdev_ms": statistics.stdev(ts) if len(ts) > 1 else 0.0,
                   "min_ms": min(ts), "max_ms": max(ts), "over_v6_fixed": statistics.mean(ts) / base}
            if name.startswith("v7_term"):
                row["over_v7_fixed"] = statistics.mean(ts) / statistics.mean(times["v7_or_m7"])
                v6_row = "v6" + name[2:]
                row["over_" + v6_row] = statistics.mean(ts) / statistics.mean(times[v6_row])
            row.update(episode.get(name, {}))
            result["variants"][name] = row
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
