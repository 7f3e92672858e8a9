"""K14 `ops.population_forward_shared` against the vmap path it replaces.

(a) One shared-minibatch population forward, n members on a (B, D0) batch,
for the stacks 8 -> 64 -> 64 -> 1, 784 -> 128 -> 10 and 376 -> 64 -> 17 (tanh
between the layers): the kernel (`ops.population_forward_shared`), and the
vmap path (`forward_shared` under `eager_on_gpu()`, what the parent commit
runs). Device events, a warm-up of each, the variants alternating round by
round in one process; a sample is --reps forwards between two events.

(b) One CEM generation of `SupervisedNE` (MSE, common minibatch of B rows)
on the first stack at popsize n, with the kernel and with the evaluation
held on the vmap path.

    python scripts/measure_population_forward_shared.py [--popsize 1024] [--batch 128] [--rounds 10]

Prints one JSON line per stack and one for the generation. Run it twice.

With --precision bf16, (a) times K15 (`ops.population_forward_shared_bf16`)
beside K14 called directly and the fp32 vmap path, and K15 with its batch
tile forced to 32 and to 64 rows where the stack's LDS rows allow it (the
measurement behind its tile rule); (b) is left out. `max_abs_diff` is then
K15 against the vmap path: bf16 rounding, not an error of the kernel.
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
    ap.add_argument("--reps", type=int, default=20, help="forwards per timed sample in (a)")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"

    from evotorch_amd import ops
    from evotorch_amd.algorithms import CEM
    from evotorch_amd.models.functional import make_functional_module
    from evotorch_amd.neuroevolution import SupervisedNE

    n, B = args.popsize, args.batch
    g = torch.Generator().manual_seed(0)
    stacks = {
        "8-64-64-1": nn.Sequential(nn.Linear(8, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)),
        "784-128-10": nn.Sequential(nn.Linear(784, 128), nn.Tanh(), nn.Linear(128, 10)),
        "376-64-17": nn.Sequential(nn.Linear(376, 64), nn.Tanh(), nn.Linear(64, 17)),
    }
    for name, net in stacks.items():
        fmodule = make_functional_module(net)
        assert fmodule._dense_stack is not None
        params = (0.1 * torch.randn(n, fmodule.parameter_count, generator=g)).cuda()
        x = torch.randn(B, fmodule._dense_stack[0][0], generator=g).cuda()

        def vmapped():
            with ops.eager_on_gpu():
                return fmodule.forward_shared(params, x)

        # the op itself: forward_shared routes only the stacks on which the kernel won here
        variants = {"kernel": lambda: ops.population_forward_shared(params, x, *fmodule._dense_stack), "vmap": vmapped}
        if args.precision == "bf16":
            mod = ops.hip_required()
            variants = {"kernel": lambda: ops.population_forward_shared_bf16(params, x, *fmodule._dense_stack),
                        "k14": variants["kernel"], "vmap": vmapped}
            for bt in (32, 64):
                try:
                    mod.population_mlp_forward_shared_bf16(params, x, *fmodule._dense_stack, bt)
                except RuntimeError:  # this tile does not fit the LDS at these widths
                    continue
                variants[f"kernel_bt{bt}"] = lambda bt=bt: mod.population_mlp_forward_shared_bf16(params, x, *fmodule._dense_stack, bt)
        max_diff = (variants["kernel"]() - variants["vmap"]()).abs().max().item()
        rows = _alternate(variants, args.rounds, args.warmup, args.reps)
        print(json.dumps({"forward": name, "precision": args.precision, "n": n, "B": B, "rounds": args.rounds,
                          "reps": args.reps, "max_abs_diff": max_diff,
                          "vmap_over_kernel": rows["vmap"]["mean_ms"] / rows["kernel"]["mean_ms"], "variants": rows}),
              flush=True)

    if args.precision == "bf16":
        return
    X, Y = torch.randn(64 * B, 8, generator=g), torch.randn(64 * B, 1, generator=g)
    generations = {}
    for kernel in (True, False):
        problem = SupervisedNE(torch.utils.data.TensorDataset(X, Y), stacks["8-64-64-1"], nn.functional.mse_loss,
                               minibatch_size=B, device="cuda:0", seed=1)
        searcher = CEM(problem, popsize=n, parenthood_ratio=0.5, stdev_init=0.1)
        if not kernel:  # hold this problem's evaluation on the vmap path, as before K14
            problem._net_obj = problem._instantiate_net().to(problem.network_device)
            problem._fmodule = make_functional_module(problem._net_obj)
            problem._fmodule._dense_stack = None
        generations["kernel" if kernel else "vmap"] = searcher.step
    rows = _alternate(generations, args.rounds, args.warmup)
    print(json.dumps({"generation": "8-64-64-1", "popsize": n, "B": B, "rounds": args.rounds, "variants": rows}),
          flush=True)


if __name__ == "__main__":
    main()
