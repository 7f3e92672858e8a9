"""Numerical cross-validation against the reference implementation: feed
IDENTICAL populations/fitnesses into both frameworks' ranking functions,
distribution gradients (Separable/Symmetric/ExpSeparable), and ClipUp/Adam
optimizers, and report max elementwise differences. Expected: <=1e-6
everywhere (the reference casts rankings to float32 internally, so fp64
inputs bottom out at fp32 epsilon). Output recorded in
profiles/crosscheck_reference.log.

The inputs and the reference's outputs are stored vectors in
tests/golden/crosscheck_reference.npz, so the check needs nothing outside
the repository:

    python scripts/crosscheck_reference.py                  # check against the stored vectors
    python scripts/crosscheck_reference.py --record REF_SRC # re-record them from a reference tree

Recording requires the reference tree (REF_SRC is its `src` directory);
ray/gymnasium are stubbed just enough to import its distributions/optimizers
modules (no reference code executes beyond the functions under test)."""

import argparse
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "crosscheck_reference.npz")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _import_reference(reference_src):
    class _T:  # generic placeholder type
        pass

    _stub("ray", remote=lambda *a, **k: (lambda f: f), is_initialized=lambda: False, ObjectRef=object)
    _stub("ray.util", ActorPool=object)
    _stub("ray.actor", ActorHandle=object)
    gym = _stub("gymnasium", Env=object, Wrapper=object, make=lambda *a, **k: None, __version__="1.0.0")
    spaces = _stub("gymnasium.spaces", Box=_T, Discrete=_T, MultiDiscrete=_T, Space=_T)
    gym.spaces = spaces
    vecutils = _stub("gymnasium.vector.utils", batch_space=lambda *a, **k: None)
    vec = _stub("gymnasium.vector", VectorEnv=_T, SyncVectorEnv=_T, utils=vecutils)
    gym.vector = vec
    _stub("gymnasium.wrappers")

    sys.path.insert(0, reference_src)
    from evotorch import distributions, optimizers
    from evotorch.tools import constraints, misc, ranking

    return types.SimpleNamespace(
        distributions=distributions, optimizers=optimizers, ranking=ranking, misc=misc, constraints=constraints
    )


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", metavar="REF_SRC", default=None,
                    help="re-record the stored vectors from the reference tree whose `src` directory is REF_SRC")
    args = ap.parse_args()

    import numpy as np
    import torch

    recording = args.record is not None
    if recording:
        if not os.path.isdir(args.record):
            sys.exit(f"reference tree not found at {args.record}")
        ref = _import_reference(args.record)
        store = {}
    else:
        ref = None
        with np.load(GOLDEN) as z:
            store = {k: z[k] for k in z.files}

    def vec(key, make):
        """A stored vector: an input shared by both sides, or a reference
        output. Computed by `make` (and stored) when recording, read back
        from the golden file otherwise."""
        if recording:
            v = make()
            v = v.detach().double() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
            store[key] = v.numpy()
            return v
        return torch.from_numpy(store[key])

    sys.path.insert(0, REPO)
    from evotorch_amd.distributions import ExpSeparableGaussian as MyExp
    from evotorch_amd.distributions import SeparableGaussian as MySep
    from evotorch_amd.distributions import SymmetricSeparableGaussian as MySym
    from evotorch_amd.optimizers import Adam as MyAdam
    from evotorch_amd.optimizers import ClipUp as MyClipUp
    from evotorch_amd.utils import ranking as my_ranking

    torch.manual_seed(0)
    L, N = 13, 24
    report = []

    fit = vec("in/fit", lambda: torch.randn(N, dtype=torch.float64))
    for method in ["centered", "linear", "nes", "normalized", "raw"]:
        for hib in (True, False):
            name = f"rank/{method}/hib={int(hib)}"
            r_ref = vec(f"ref/{name}", lambda: ref.ranking.rank(fit, ranking_method=method, higher_is_better=hib))
            r_my = my_ranking.rank(fit, method, higher_is_better=hib)
            report.append((name, (r_ref.double() - r_my.double()).abs().max().item()))

    mu = vec("in/mu", lambda: torch.randn(L, dtype=torch.float64))
    sigma = vec("in/sigma", lambda: torch.rand(L, dtype=torch.float64) + 0.5)
    samples = vec("in/samples", lambda: mu + sigma * torch.randn(N, L, dtype=torch.float64))
    fitn = vec("in/fitn", lambda: torch.randn(N, dtype=torch.float64))

    def ref_grads(name, keys, make):
        """Reference gradient dict, one stored vector per key."""
        g = make() if recording else None
        if recording:
            assert sorted(g) == sorted(keys), sorted(g)
        return {k: vec(f"ref/{name}/{k}", lambda: g[k]) for k in keys}

    for div in [None, "num_solutions", "total_weight"]:
        params = {"mu": mu.clone(), "sigma": sigma.clone()}
        if div:
            params.update(divide_mu_grad_by=div, divide_sigma_grad_by=div)
        g_ref = ref_grads(f"Sep/div={div}", ["mu", "sigma"], lambda: ref.distributions.SeparableGaussian(dict(params)).compute_gradients(
            samples, fitn, objective_sense="max", ranking_method="centered"))
        g_my = MySep(dict(params)).compute_gradients(samples, fitn, objective_sense="max", ranking_method="centered")
        assert sorted(g_my) == sorted(g_ref), sorted(g_my)
        for k in sorted(g_ref):
            report.append((f"Sep/div={div}/{k}", (g_ref[k] - g_my[k]).abs().max().item()))

    # symmetric: reference interleaves (+,-) pairs, this framework uses the
    # halves layout — remap before comparing
    d_half = N // 2
    base = vec("in/sym_base", lambda: torch.randn(d_half, L, dtype=torch.float64))
    plus, minus = mu + sigma * base, mu - sigma * base
    ref_samples = torch.empty(N, L, dtype=torch.float64)
    ref_samples[0::2], ref_samples[1::2] = plus, minus
    my_samples = torch.cat([plus, minus])
    f_plus = vec("in/sym_f_plus", lambda: torch.randn(d_half, dtype=torch.float64))
    f_minus = vec("in/sym_f_minus", lambda: torch.randn(d_half, dtype=torch.float64))
    ref_fit = torch.empty(N, dtype=torch.float64)
    ref_fit[0::2], ref_fit[1::2] = f_plus, f_minus
    my_fit = torch.cat([f_plus, f_minus])
    params = {"mu": mu.clone(), "sigma": sigma.clone(),
              "divide_mu_grad_by": "num_directions", "divide_sigma_grad_by": "num_directions"}
    g_ref = ref_grads("Sym", ["mu", "sigma"], lambda: ref.distributions.SymmetricSeparableGaussian(dict(params)).compute_gradients(
        ref_samples, ref_fit, objective_sense="max", ranking_method="centered"))
    g_my = MySym(dict(params)).compute_gradients(my_samples, my_fit, objective_sense="max", ranking_method="centered")
    assert sorted(g_my) == sorted(g_ref), sorted(g_my)
    for k in sorted(g_ref):
        report.append((f"Sym/{k}", (g_ref[k] - g_my[k]).abs().max().item()))

    g_ref = ref_grads("ExpSep-nes", ["mu", "sigma"], lambda: ref.distributions.ExpSeparableGaussian(
        {"mu": mu.clone(), "sigma": sigma.clone()}).compute_gradients(samples, fitn, objective_sense="min", ranking_method="nes"))
    g_my = MyExp({"mu": mu.clone(), "sigma": sigma.clone()}).compute_gradients(samples, fitn, objective_sense="min", ranking_method="nes")
    assert sorted(g_my) == sorted(g_ref), sorted(g_my)
    for k in sorted(g_ref):
        report.append((f"ExpSep-nes/{k}", (g_ref[k] - g_my[k]).abs().max().item()))

    # stdev-control clamping (modify_tensor drives PGPE's stdev_max_change)
    from evotorch_amd.utils import modify_tensor as my_modify
    from evotorch_amd.utils import stdev_from_radius as my_sfr

    orig = vec("in/modify_orig", lambda: torch.rand(40, dtype=torch.float64) + 0.5)
    target = vec("in/modify_target", lambda: orig * torch.empty(40, dtype=torch.float64).uniform_(0.3, 3.0))
    for kwargs in (dict(lb=0.6, ub=2.0), dict(max_change=0.2), dict(lb=0.7, ub=1.8, max_change=0.3)):
        name = f"modify_tensor/{sorted(kwargs)}"
        a = vec(f"ref/{name}", lambda: ref.misc.modify_tensor(orig, target, **kwargs))
        b = my_modify(orig, target, **kwargs)
        report.append((name, (a - b).abs().max().item()))
    a = vec("ref/stdev_from_radius", lambda: ref.misc.stdev_from_radius(2.25, 6409))
    report.append(("stdev_from_radius", abs(a.item() - my_sfr(2.25, 6409))))

    # constraint penalization helpers
    from evotorch_amd.utils import constraints as my_constraints

    cx = vec("in/cx", lambda: torch.randn(64, dtype=torch.float64) * 3)
    for op in ("<=", ">="):
        a = vec(f"ref/violation/{op}", lambda: ref.constraints.violation(lhs=cx, comparison=op, rhs=1.0))
        b = my_constraints.violation(lhs=cx, comparison=op, rhs=1.0)
        report.append((f"violation/{op}", (a - b).abs().max().item()))
        a = vec(f"ref/log_barrier/{op}", lambda: ref.constraints.log_barrier(lhs=cx, comparison=op, rhs=1.0, penalty_sign="-"))
        b = my_constraints.log_barrier(lhs=cx, comparison=op, rhs=1.0, penalty_sign="-")
        finite = torch.isfinite(a)
        assert torch.equal(torch.isfinite(b), finite)  # same -inf pattern
        report.append((f"log_barrier/{op}", (a[finite] - b[finite]).abs().max().item() if finite.any() else 0.0))
    a = vec("ref/penalty", lambda: ref.constraints.penalty(
        lhs=cx, comparison="<=", rhs=1.0, penalty_sign="-", linear=2.0, step=5.0, exp=2.0, exp_inf=100.0))
    b = my_constraints.penalty(lhs=cx, comparison="<=", rhs=1.0, penalty_sign="-", linear=2.0, step=5.0, exp=2.0, exp_inf=100.0)
    report.append(("penalty", (a - b).abs().max().item()))

    g_seq = [vec(f"in/opt_grad/{i}", lambda: torch.randn(L, dtype=torch.float64)) for i in range(5)]
    pairs = [
        ("ClipUp/5steps",
         lambda: ref.optimizers.ClipUp(solution_length=L, dtype=torch.float64, stepsize=0.1, max_speed=0.2),
         MyClipUp(solution_length=L, dtype=torch.float64, stepsize=0.1, max_speed=0.2)),
        ("Adam/5steps",
         lambda: ref.optimizers.Adam(solution_length=L, dtype=torch.float64, stepsize=0.01),
         MyAdam(solution_length=L, dtype=torch.float64, stepsize=0.01)),
    ]
    for name, make_ref_o, my_o in pairs:
        ref_o = make_ref_o() if recording else None
        worst = 0.0
        for i, g in enumerate(g_seq):
            step_ref = vec(f"ref/{name}/{i}", lambda: ref_o.ascent(g))
            worst = max(worst, (step_ref - my_o.ascent(g)).abs().max().item())
        report.append((name, worst))

    if recording:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        np.savez(GOLDEN, **store)
        print(f"recorded {len(store)} vectors to {os.path.relpath(GOLDEN, REPO)}")

    failures = 0
    for n, d in report:
        ok = d <= 1e-6  # False for NaN too
        status = "OK " if ok else "FAIL"
        if not ok:
            failures += 1
        print(f"{status} {n:28s} maxdiff {d:.3e}")
    print("RESULT:", "all within 1e-6 of the reference" if failures == 0 else f"{failures} mismatches")
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
