"""Record tests/golden/rollout_v7_bits_t50.npz: fitness, sum and sumsq of the
v7 rollout kernel for the 50-step cases of
tests/test_gpu_rollout_v7_butterfly.py, with that test's own inputs.

Run it on an MI355X with the build whose bits are to be kept (the fixture in
the repository was recorded from the commit before the select-free
butterfly):

    python scripts/record_rollout_v7_bits_t50.py [OUT.npz]
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_rollout_v7_butterfly as cases  # noqa: E402


def main():
    assert torch.cuda.is_available(), "recording needs the GPU kernel"
    import evotorch_amd._C as C

    os.environ.pop("EVOTORCH_AMD_ROLLOUT_V6", None)
    out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
    arrays = {}
    for n, steps in cases.GOLDEN_CASES:
        first = cases.run_kernel(C, cases._random_params()[:n], steps)
        again = cases.run_kernel(C, cases._random_params()[:n], steps)
        for name, x, y in zip(("fitness", "sum", "sumsq"), first, again):
            assert torch.isfinite(x).all(), (name, n, steps)
            assert torch.equal(x, y), f"{name} of n={n} T={steps} does not repeat"
            arrays[f"{name}_n{n}_t{steps}"] = x.numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"wrote {out}: " + ", ".join(f"{k}{v.shape}" for k, v in arrays.items()))


if __name__ == "__main__":
    main()
