"""K16 `ops.population_forward_recurrent` against the vmap path it replaces.

One policy step with state at n members for the stacks
`RNN(32, 16) >> Linear(16, 8)`, `LSTM(376, 64) >> Linear(64, 17)` and
`Linear(376, 64) >> Tanh() >> LSTM(64, 64) >> Linear(64, 17)`, through
`models.Policy`: with `recurrent_kernel=True`, and on the vmap path (the
default). Each sample restores the same given state first, so both variants
time the stateful step a rollout repeats. Device events, a warm-up of each,
the variants alternating round by round in one process; a sample is --reps
steps between two events, since one step is tens of microseconds.

    python scripts/measure_population_forward_recurrent.py [--popsize 2048] [--rounds 10]

Prints one JSON line per stack. Run it twice.
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from measure_population_forward import _alternate  # noqa: E402

STACKS = {
    "rnn 32-16 >> 8": "RNN(32, 16) >> Linear(16, 8)",
    "lstm 376-64 >> 17": "LSTM(376, 64) >> Linear(64, 17)",
    "376-64 >> lstm 64 >> 17": "Linear(376, 64) >> Tanh() >> LSTM(64, 64) >> Linear(64, 17)",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="steps per timed sample")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"

    from evotorch_amd.models import Policy

    n = args.popsize
    g = torch.Generator().manual_seed(0)
    for name, net in STACKS.items():
        policies = {"kernel": Policy(net, recurrent_kernel=True), "vmap": Policy(net)}
        kinds, widths, _, _, state_index = policies["kernel"]._fmodule._recurrent_stack
        params = (0.1 * torch.randn(n, policies["kernel"].parameter_count, generator=g)).cuda()
        obs = torch.randn(n, widths[0], generator=g).cuda()
        for policy in policies.values():
            policy.set_parameters(params)
            policy(obs)  # from no state: leaves the state every timed step starts from
        start = {key: policy.h for key, policy in policies.items()}
        assert list(start["kernel"]) == list(start["vmap"]) == [state_index]

        def step(key):
            policies[key]._state = start[key]
            return policies[key](obs)

        variants = {key: (lambda key=key: step(key)) for key in policies}
        max_diff = (variants["kernel"]() - variants["vmap"]()).abs().max().item()
        rows = _alternate(variants, args.rounds, args.warmup, args.reps)
        print(json.dumps({"step": name, "n": n, "rounds": args.rounds, "reps": args.reps, "max_abs_diff": max_diff,
                          "vmap_over_kernel": rows["vmap"]["mean_ms"] / rows["kernel"]["mean_ms"], "variants": rows}),
              flush=True)


if __name__ == "__main__":
    main()
