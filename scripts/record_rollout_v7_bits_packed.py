"""Record tests/golden/rollout_v7_bits_packed.npz: fitness, sum and sumsq of
the v7 rollout kernel for the cases of tests/test_gpu_rollout_v7_packed.py
(row pairs across the live boundary, and the clamp of tanh_fast), with that
test's own inputs.

Run it on an MI355X with the build whose bits are to be kept (the fixture in
the repository was recorded from the commit before the packed epilogue):

    python scripts/record_rollout_v7_bits_packed.py [OUT.npz]
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_rollout_v7_packed as cases  # noqa: E402


def main():
    assert torch.cuda.is_available(), "recording needs the GPU kernel"
    import evotorch_amd._C as C

    os.environ.pop("EVOTORCH_AMD_ROLLOUT_V6", None)
    out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
    arrays = {}
    for kind, n in cases.GOLDEN_CASES:
        first = cases.run_kernel(C, kind, 0, n)
        again = cases.run_kernel(C, kind, 0, n)
        for name, x, y in zip(("fitness", "sum", "sumsq"), first, again):
            assert torch.isfinite(x).all(), (name, kind, n)
            assert torch.equal(x, y), f"{name} of {kind} n={n} does not repeat"
            arrays[f"{name}_{kind}_n{n}"] = x.numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"wrote {out}: " + ", ".join(f"{k}{v.shape}" for k, v in arrays.items()))


if __name__ == "__main__":
    main()
