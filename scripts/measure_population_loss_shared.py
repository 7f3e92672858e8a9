"""K17 `ops.population_loss_shared` against the line it replaces.

(a) The mean loss of n members on one shared minibatch (B rows), for
8 -> 64 -> 64 -> 1 with MSE and 376 -> 64 -> 17 with cross-entropy in fp32,
and 784 -> 128 -> 10 with cross-entropy in bf16 (tanh between the layers):
the fused kernel, and today's line, the K14 (or K15) forward followed by the
vmapped torch loss. Device events, a warm-up of each, the variants
alternating round by round in one process; a sample is --reps calls between
two events.

(b) One CEM generation of `SupervisedNE` (8 -> 64 -> 64 -> 1, `nn.MSELoss()`,
common minibatch of B rows) at popsize n: fused, and with the same loss held
behind a lambda, which keeps the evaluation on the K14 forward and the
vmapped loss.

    python scripts/measure_population_loss_shared.py [--popsize 1024] [--batch 128] [--rounds 10]

Prints one JSON line per stack and one for the generation. Run it twice.
"""

import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from measure_population_forward import _alternate  # noqa: E402  (the same timing loop as K13's script)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed sample in (a)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"

    from evotorch_amd import ops
    from evotorch_amd.algorithms import CEM
    from evotorch_amd.models.functional import make_functional_module
    from evotorch_amd.neuroevolution import SupervisedNE

    n, B = args.popsize, args.batch
    g = torch.Generator().manual_seed(0)
    small = nn.Sequential(nn.Linear(8, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
    cases = {  # name -> (net, loss, precision)
        "8-64-64-1": (small, "mse", "fp32"),
        "376-64-17": (nn.Sequential(nn.Linear(376, 64), nn.Tanh(), nn.Linear(64, 17)), "cross_entropy", "fp32"),
        "784-128-10": (nn.Sequential(nn.Linear(784, 128), nn.Tanh(), nn.Linear(128, 10)), "cross_entropy", "bf16"),
    }
    for name, (net, loss, precision) in cases.items():
        fmodule = make_functional_module(net)
        widths = fmodule._dense_stack[0]
        params = (0.1 * torch.randn(n, fmodule.parameter_count, generator=g)).cuda()
        x = torch.randn(B, widths[0], generator=g).cuda()
        if loss == "mse":
            y, loss_func = torch.randn(B, widths[-1], generator=g).cuda(), nn.functional.mse_loss
        else:
            y, loss_func = torch.randint(0, widths[-1], (B,), generator=g).cuda(), nn.functional.cross_entropy
        forward = ops.population_forward_shared_bf16 if precision == "bf16" else ops.population_forward_shared

        def fused():
            return ops.population_loss_shared(params, x, y, *fmodule._dense_stack, loss=loss, precision=precision)

        def unfused():
            return torch.func.vmap(lambda p: loss_func(p, y))(forward(params, x, *fmodule._dense_stack))

        max_diff = (fused() - unfused()).abs().max().item()
        rows = _alternate({"fused": fused, "unfused": unfused}, args.rounds, args.warmup, args.reps)
        print(json.dumps({"loss": name, "kind": loss, "precision": precision, "n": n, "B": B, "rounds": args.rounds,
                          "reps": args.reps, "max_abs_diff": max_diff,
                          "unfused_over_fused": rows["unfused"]["mean_ms"] / rows["fused"]["mean_ms"], "variants": rows}),
              flush=True)

    X, Y = torch.randn(64 * B, 8, generator=g), torch.randn(64 * B, 1, generator=g)
    generations = {}
    for fused in (True, False):
        mse = nn.MSELoss()
        problem = SupervisedNE(torch.utils.data.TensorDataset(X, Y), small, mse if fused else (lambda p, t: mse(p, t)),
                               minibatch_size=B, device="cuda:0", seed=1)
        assert (problem._fused_loss_kind() == "mse") == fused
        generations["fused" if fused else "unfused"] = CEM(problem, popsize=n, parenthood_ratio=0.5, stdev_init=0.1).step
    rows = _alternate(generations, args.rounds, args.warmup)
    print(json.dumps({"generation": "8-64-64-1", "popsize": n, "B": B, "rounds": args.rounds,
                      "unfused_over_fused": rows["unfused"]["mean_ms"] / rows["fused"]["mean_ms"], "variants": rows}),
          flush=True)


if __name__ == "__main__":
    main()
