"""Op dispatch: eager (CPU / reference) implementations + HIP kernel routing.

Every hot op of the framework goes through this module. The contract:

* On CPU tensors: run the eager PyTorch implementation below (these are the
  numerics references the HIP kernels are tested against).
* On ROCm (``cuda``) tensors: run the hand-written CDNA4 HIP kernel from the
  in-tree extension ``evotorch_amd._C``. If the extension is missing on a
  machine that has a GPU, we raise loudly instead of silently falling back
  (the eager path would hide a broken native build).

Kernel inventory (docs/kernels.md): K1 sample_gaussian / affine_from_noise,
K2 fused_rank (routed from utils/ranking.py), K3 es_gradients /
snes_gradients, K4 clipup_step / adam_step, K4b gaussian_clipup_update, K12
obsnorm_pack / obsnorm_merge, K5 cma_update_c, K5b potrf_tile,
K7 pareto_ranks / domination_counts, K9 mapelites_assign (routed from
algorithms/mapelites.py), K10+K11 rollout_linear (called from
neuroevolution/synthetic.py).

The launchers check every operand (ops/hip/check.h): dense, on the primary
tensor's device, of its dtype and of exactly the length the kernel reads.
The casts below hand them what they expect; `hip_for` is the one routing
decision.
"""

import contextlib
import functools
import os
from typing import Optional, Tuple

import torch

__all__ = [
    "affine_from_noise",
    "eager_on_gpu",
    "hip_available",
    "hip_for",
    "hip_required",
    "load_hip",
    "seed_from_generator",
    "sample_gaussian",
    "es_gradients",
    "snes_gradients",
    "clipup_step_",
    "gaussian_clipup_update",
    "obsnorm_merge_",
    "obsnorm_pack_",
    "unfused_generation_tail",
    "fused_tail_for",
    "GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH",
    "fused_adam_step_",
    "pareto_ranks",
    "domination_counts",
    "cma_update_c_",
]


@functools.lru_cache(maxsize=None)
def load_hip():
    """Load the in-tree HIP extension (returns None on failure, caching the
    outcome)."""
    try:
        import evotorch_amd._C as _C  # built in-tree by setup_hip.py / __graft_entry__.build()

        return _C
    except ImportError:
        return None


def hip_available() -> bool:
    return load_hip() is not None


def hip_required():
    """The HIP extension, or a loud error on a GPU machine without it."""
    mod = load_hip()
    if mod is None:
        raise RuntimeError(
            "evotorch_amd._C (the gfx950 HIP extension) is not built, but a ROCm GPU "
            "tensor reached the op dispatch layer. Build it in-tree with "
            "`python setup_hip.py build_ext --inplace` (or __graft_entry__.build()). "
            "Refusing to silently fall back to eager PyTorch on GPU."
        )
    return mod


_EAGER_ENV = "EVOTORCH_AMD_ALLOW_EAGER_GPU"  # escape hatch for debugging and reference runs only


def hip_for(t: torch.Tensor):
    """The extension when `t` is a ROCm tensor that must take the HIP path
    (loud error if it is not built), else None: CPU tensors, and ROCm
    tensors while the eager escape hatch is on, run the eager reference."""
    if t.device.type == "cuda" and os.environ.get(_EAGER_ENV, "0") != "1":
        return hip_required()
    return None


@contextlib.contextmanager
def eager_on_gpu():
    """Route ROCm tensors to the eager references inside the block; the
    environment is left exactly as it was found."""
    previous = os.environ.get(_EAGER_ENV)
    os.environ[_EAGER_ENV] = "1"
    try:
        yield
    finally:
        if previous is None:
            del os.environ[_EAGER_ENV]
        else:
            os.environ[_EAGER_ENV] = previous


_fused_tail = [True]


@contextlib.contextmanager
def unfused_generation_tail():
    """Run the generation tail (distribution update, obs-norm merge and
    env-blob packing) through the chains of separate launches that the
    fused ops replace. The chains are the fused ops' oracle: both give the
    same bits."""
    previous = _fused_tail[0]
    _fused_tail[0] = False
    try:
        yield
    finally:
        _fused_tail[0] = previous


def fused_tail_for(t: torch.Tensor):
    """The extension when `t` is an fp32 ROCm tensor and the fused
    generation tail is on, else None (the caller runs its chain)."""
    if _fused_tail[0] and t.dtype == torch.float32:
        return hip_for(t)
    return None


def _dense(like: torch.Tensor, *operands: torch.Tensor):
    # what the launchers accept beside `like`: its dtype, no strides
    return [t.to(like.dtype).contiguous() for t in operands]


_SPLITMIX_INC = 0x9E3779B97F4A7C15
_seed_fallback_counter = [0x1234ABCD]

def splitmix64(x: int) -> int:
    x = (x + _SPLITMIX_INC) & 0xFFFFFFFFFFFFFFFF
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return (z ^ (z >> 31)) & 0x7FFFFFFFFFFFFFFF


def seed_from_generator(generator: Optional[torch.Generator], device: torch.device) -> int:
    """Derive a fresh 63-bit seed deterministically from the generator's OWN
    state — no global bookkeeping, no device sync.

    CUDA generators: PyTorch tracks the philox (seed, offset) pair host-side,
    so get_offset()/set_offset() advance the generator without touching the
    GPU; the returned seed is splitmix64(initial_seed xor golden*offset).
    Two generators seeded identically produce identical seed sequences, and
    reseeding (manual_seed resets offset to 0) restarts the sequence.

    CPU generators: a single host randint draw (stateful, cheap).

    (An earlier version kept a module dict keyed by id(generator); after a
    generator was garbage collected its id could be reused by a NEW
    generator, silently resuming the dead one's counter. Generator-intrinsic
    state cannot alias.)"""
    if generator is not None:
        if generator.device.type == "cuda":
            off = int(generator.get_offset())
            generator.set_offset(off + 4)
            mixed = (int(generator.initial_seed()) ^ ((off + 1) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
            return splitmix64(mixed)
        return int(torch.randint(0, 2**62, (1,), generator=generator).item())
    _seed_fallback_counter[0] += 1
    return splitmix64(_seed_fallback_counter[0])


# ============================================================================
# K1 — Gaussian population sampling
# ============================================================================


def sample_gaussian(
    out: torch.Tensor,
    mu: torch.Tensor,
    sigma: torch.Tensor,
    *,
    symmetric: bool = False,
    generator: Optional[torch.Generator] = None,
    seed: Optional[int] = None,
    row_offset: int = 0,
) -> torch.Tensor:
    """Fill `out` (N×L) with x = mu + sigma * z. With symmetric=True, rows
    [0, N/2) hold mu + sigma*z and rows [N/2, N) the mirrored mu - sigma*z
    (halves layout — see evotorch_amd/distributions.py docstring).

    Counter-addressed mode (`seed` given): row r of `out` (a direction row
    for symmetric sampling) draws from philox stream `row_offset + r` with
    the counter walking the row — the SAME values regardless of how the
    virtual population is partitioned into row blocks (sharding across
    ranks, or chunking in the streaming large-L gradient path), and
    identical on CPU (numpy philox reference) and GPU."""
    if out.ndim != 2:
        raise ValueError(f"expected a 2-D population, got shape {tuple(out.shape)}")
    n = out.shape[0]
    if symmetric and n % 2 != 0:
        raise ValueError("symmetric sampling requires even popsize")
    mod = hip_for(out)
    if mod is not None:
        if seed is None:  # a fresh seed from the generator; row_offset addresses seeded streams only
            seed, row_offset = seed_from_generator(generator, out.device), 0
        mod.sample_gaussian(out, *_dense(out, mu, sigma), bool(symmetric), int(seed), int(row_offset))
        return out
    if seed is not None:
        # philox-exact eager reference (matches the kernel bit-for-bit in fp32)
        from ..neuroevolution.philox_ref import philox_normals_2d

        z = philox_normals_2d(int(seed), int(row_offset), n // 2 if symmetric else n, out.shape[1])
        return _affine_eager(out, z.to(device=out.device), mu, sigma, symmetric)
    # eager reference
    if symmetric:
        half = out[: n // 2]
        half.normal_(generator=generator)
        half.mul_(sigma).add_(mu)
        torch.sub(2.0 * mu, half, out=out[n // 2 :])
    else:
        out.normal_(generator=generator)
        out.mul_(sigma).add_(mu)
    return out


def affine_from_noise(
    out: torch.Tensor,
    z: torch.Tensor,
    mu: torch.Tensor,
    sigma: torch.Tensor,
    *,
    symmetric: bool,
) -> torch.Tensor:
    """x = mu + sigma*z from PRE-GENERATED fp32 standard normals (z filled
    counter-addressed on a side stream, hidden behind evaluation and the
    gradient all-reduce). Bitwise-identical to `sample_gaussian` with the
    same seed/row_offset: both compute fmaf(sigma, z, mu) in fp32."""
    mod = hip_for(out)
    if mod is not None:
        mod.affine_from_noise(out, z, *_dense(out, mu, sigma), bool(symmetric))
        return out
    return _affine_eager(out, z, mu, sigma, symmetric)


def _affine_eager(out, z, mu, sigma, symmetric):
    n = out.shape[0]
    rows = n // 2 if symmetric else n
    mu32 = mu.to(torch.float32)
    s32 = sigma.to(torch.float32)
    plus = (mu32 + s32 * z.reshape(rows, -1)).to(out.dtype)
    if symmetric:
        out[:rows] = plus
        out[rows:] = (2.0 * mu32 - plus.to(torch.float32)).to(out.dtype)
    else:
        out.copy_(plus)
    return out


# ============================================================================
# K3 — fused ES gradient reductions (N×L → L)
# ============================================================================


def es_gradients(
    samples: torch.Tensor,
    mu: torch.Tensor,
    sigma: torch.Tensor,
    weights: torch.Tensor,
    *,
    symmetric: bool,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain/antithetic ES gradients of a separable Gaussian.

    Non-symmetric (reference distributions.py:548-579):
        mu_grad[l]    = Σ_i w_i · (x_il − μ_l)
        sigma_grad[l] = Σ_i w_i · ((x_il − μ_l)² − σ_l²) / σ_l

    Symmetric halves layout (reference distributions.py:708-773 with the
    interleaved layout mapped to halves):
        noise_d       = x_d − μ            (d < N/2; x_{d+N/2} = μ − noise_d)
        mu_grad[l]    = Σ_d (w⁺_d − w⁻_d)/2 · noise_dl
        sigma_grad[l] = Σ_d (w⁺_d + w⁻_d)/2 · (noise_dl² − σ_l²)/σ_l
    """
    mod = hip_for(samples)
    if mod is not None:
        return mod.es_gradients(samples, *_dense(samples, mu, sigma, weights), bool(symmetric))
    w_mu = w_sigma = weights.to(torch.float32)
    if symmetric:
        d = samples.shape[0] // 2
        samples, w_plus, w_minus = samples[:d], w_mu[:d], w_mu[d:]
        w_mu, w_sigma = (w_plus - w_minus) / 2.0, (w_plus + w_minus) / 2.0
    noises = samples.to(torch.float32) - mu.to(torch.float32)
    sigma32 = sigma.to(torch.float32)
    mu_grad = w_mu @ noises
    sigma_grad = w_sigma @ ((noises**2 - sigma32**2) / sigma32)
    return mu_grad.to(samples.dtype), sigma_grad.to(samples.dtype)


def snes_gradients(
    samples: torch.Tensor,
    mu: torch.Tensor,
    sigma: torch.Tensor,
    weights: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """SNES natural gradients (reference distributions.py:783-793):
        mu_grad[l]    = Σ_i w_i · (x_il − μ_l)
        sigma_grad[l] = Σ_i w_i · (z_il² − 1),  z = (x − μ)/σ
    """
    mod = hip_for(samples)
    if mod is not None:
        return mod.snes_gradients(samples, *_dense(samples, mu, sigma, weights))
    noises = samples.to(torch.float32) - mu.to(torch.float32)
    raw = noises / sigma.to(torch.float32)
    w = weights.to(torch.float32)
    mu_grad = w @ noises
    sigma_grad = w @ (raw**2 - 1.0)
    return mu_grad.to(samples.dtype), sigma_grad.to(samples.dtype)


# ============================================================================
# K4 — optimizer steps (fused on device)
# ============================================================================


def clipup_step_(
    velocity: torch.Tensor,
    grad: torch.Tensor,
    *,
    step_size: float,
    max_speed: float,
    momentum: float = 0.9,
) -> torch.Tensor:
    """In-place ClipUp ascent step (Toklu et al. 2020; reference
    optimizers.py:231-357). Normalizes grad to unit L2, takes a step of
    `step_size`, adds momentum-scaled velocity, clips the velocity norm to
    `max_speed`. Returns the updated velocity (= the ascent step)."""
    mod = hip_for(velocity)
    if mod is not None:
        mod.clipup_step(velocity, *_dense(velocity, grad), float(step_size), float(max_speed), float(momentum))
        return velocity
    g32 = grad.to(torch.float32)
    gnorm = torch.linalg.vector_norm(g32)
    step = g32 * (step_size / torch.clamp(gnorm, min=1e-30))
    v32 = velocity.to(torch.float32) * momentum + step
    vnorm = torch.linalg.vector_norm(v32)
    scale = torch.clamp(max_speed / torch.clamp(vnorm, min=1e-30), max=1.0)
    v32 = v32 * scale
    velocity.copy_(v32.to(velocity.dtype))
    return velocity


GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH = 65536  # one block; kUpdateMaxLength of es_kernels.hip


def gaussian_clipup_update(
    mu: torch.Tensor,
    sigma: torch.Tensor,
    velocity: torch.Tensor,
    mu_grad: torch.Tensor,
    sigma_grad: torch.Tensor,
    *,
    step_size: float,
    max_speed: float,
    momentum: float = 0.9,
    sigma_lr: float,
    stdev_min: Optional[float] = None,
    stdev_max: Optional[float] = None,
    stdev_max_change: Optional[float] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The distribution update of a separable Gaussian under ClipUp:
    `velocity` takes one ClipUp step along `mu_grad` in place (as
    `clipup_step_`), and fresh ``(mu + velocity, sigma')`` are returned,
    where ``sigma' = sigma + sigma_lr * sigma_grad`` held inside the scalar
    stdev bounds exactly as `utils.modify_tensor` holds it.

    fp32 ROCm vectors up to GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH elements take
    ONE kernel launch; anything else runs the chain of launches below. Both
    give the same bits. No host sync either way (hipGraph-capturable)."""
    mod = fused_tail_for(mu)
    if (
        mod is not None
        and mu.numel() <= GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH
        and all(t.dtype == torch.float32 and t.device == mu.device for t in (sigma, velocity, mu_grad, sigma_grad))
        and velocity.is_contiguous()
    ):
        new_mu, new_sigma = mod.gaussian_clipup_update(
            *_dense(mu, mu, sigma),
            velocity,
            *_dense(mu, mu_grad, sigma_grad),
            float(step_size),
            float(momentum),
            float(max_speed),
            float(sigma_lr),
            None if stdev_min is None else float(stdev_min),
            None if stdev_max is None else float(stdev_max),
            None if stdev_max_change is None else float(stdev_max_change),
        )
        return new_mu, new_sigma
    from ..utils.misc import modify_tensor

    clipup_step_(velocity, mu_grad, step_size=step_size, max_speed=max_speed, momentum=momentum)
    new_mu = mu + velocity
    new_sigma = torch.add(sigma, sigma_grad, alpha=float(sigma_lr))
    if stdev_min is not None or stdev_max is not None or stdev_max_change is not None:
        new_sigma = modify_tensor(sigma, new_sigma, lb=stdev_min, ub=stdev_max, max_change=stdev_max_change)
    return new_mu, new_sigma


# ============================================================================
# K12 — observation-normalization statistics
# ============================================================================


def obsnorm_merge_(count: torch.Tensor, total: torch.Tensor, total_sq: torch.Tensor, c, s: torch.Tensor, ss: torch.Tensor):
    """``count += c; total += s; total_sq += ss`` on RunningNorm's state.
    `c` is a host number or a one-element tensor; a device tensor is read
    on the device (no host sync). One launch on fp32 ROCm state."""
    mod = fused_tail_for(total)
    c_is_tensor = isinstance(c, torch.Tensor)
    if (
        mod is not None
        and count.dtype == torch.float64
        and count.device == total.device
        and total_sq.dtype == torch.float32
        and s.shape == total.shape
        and ss.shape == total.shape
        and total.is_contiguous()
        and total_sq.is_contiguous()
        and total.numel() > 0
        and (not c_is_tensor or (c.device == total.device and c.numel() == 1 and c.dtype in (torch.float32, torch.float64)))
    ):
        mod.obsnorm_merge(count, total, total_sq, 0.0 if c_is_tensor else float(c), c if c_is_tensor else None, *_dense(total, s, ss))
        return
    if c_is_tensor:
        count += c.to(count.device, torch.float64)
    else:
        count += float(c)
    total += s
    total_sq += ss


def obsnorm_pack_(blob: torch.Tensor, offset: int, count: torch.Tensor, total: torch.Tensor, total_sq: torch.Tensor, min_variance: float) -> bool:
    """Write RunningNorm's mean and stdev (fp32) into
    ``blob[offset : offset + 2 * O]`` in one launch, straight from the
    running sums. Returns False, having done nothing, where the fused path
    does not apply (the caller then goes through RunningNorm's properties)."""
    mod = fused_tail_for(blob)
    if (
        mod is None
        or count.dtype != torch.float64
        or total.dtype != torch.float32
        or total_sq.dtype != torch.float32
        or not (count.device == total.device == total_sq.device == blob.device)
        or not (blob.is_contiguous() and total.is_contiguous() and total_sq.is_contiguous())
    ):
        return False
    mod.obsnorm_pack(count, total, total_sq, float(min_variance), blob, int(offset))
    return True


def fused_adam_step_(
    param_step_out: torch.Tensor,
    grad: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    *,
    step_count: int,
    stepsize: float,
    beta1: float = 0.9,
    beta2: float = 0.999,
    epsilon: float = 1e-8,
) -> torch.Tensor:
    """In-place Adam *ascent* step: updates moments m, v and writes the
    additive step into `param_step_out`."""
    mod = hip_for(grad)
    if mod is not None:
        mod.adam_step(param_step_out, *_dense(param_step_out, grad), m, v, int(step_count), float(stepsize), float(beta1), float(beta2), float(epsilon))
        return param_step_out
    g32 = grad.to(torch.float32)
    m32 = m.to(torch.float32) * beta1 + (1.0 - beta1) * g32
    v32 = v.to(torch.float32) * beta2 + (1.0 - beta2) * g32 * g32
    m.copy_(m32.to(m.dtype))
    v.copy_(v32.to(v.dtype))
    mhat = m32 / (1.0 - beta1**step_count)
    vhat = v32 / (1.0 - beta2**step_count)
    param_step_out.copy_((stepsize * mhat / (vhat.sqrt() + epsilon)).to(param_step_out.dtype))
    return param_step_out


# ============================================================================
# K7 — NSGA-II non-dominated sorting
# ============================================================================


def domination_counts(utils: torch.Tensor) -> torch.Tensor:
    """Per solution: how many others dominate it. `utils` is (N, M) with
    higher-is-better columns."""
    mod = hip_for(utils)
    if mod is not None:
        return mod.domination_counts(utils).to(torch.int64)
    a = utils.unsqueeze(1)
    b = utils.unsqueeze(0)
    dom = (a >= b).all(dim=-1) & (a > b).any(dim=-1)
    return dom.sum(dim=0).to(torch.int64)


def pareto_ranks(utils: torch.Tensor, min_assigned: Optional[int] = None) -> torch.Tensor:
    """Front index per solution (0 = non-dominated front), computed on GPU
    by count + front peeling without the N x N matrix. With
    `min_assigned`, peeling stops once that many solutions hold final
    ranks (take_best(n) only needs the fronts crossing n); the rest get a
    shared beyond-last rank."""
    mod = hip_for(utils)
    if mod is not None:
        return mod.pareto_ranks(utils, int(min_assigned or 0))
    from ..core import _compute_pareto_ranks_eager

    ranks, _ = _compute_pareto_ranks_eager(utils, crowdsort=False, min_assigned=min_assigned)
    return ranks


# ============================================================================
# K5 — fused CMA-ES covariance update
# ============================================================================


def cma_update_c_(
    C: torch.Tensor,
    y: torch.Tensor,
    w_adj: torch.Tensor,
    p_c: torch.Tensor,
    hs_f: torch.Tensor,
    *,
    c1: float,
    cmu: float,
    cc: float,
) -> torch.Tensor:
    """In-place C = scale·C + c1·pc pcᵀ + cμ·Yᵀdiag(w)Y, exactly
    symmetric, with scale = 1 + c1·(1−hs)·cc·(2−cc) − c1 − cμ·Σw computed
    from DEVICE scalars (no host sync per generation).

    On GPU this is ONE fused pass over C (ops/hip/cma.hip — see that file
    for why fp32 VALU, not MFMA, is the right tool at CMA-ES shapes); the
    eager reference is the reference-parity torch chain (cmaes.py:547-553)
    plus explicit symmetrization."""
    wsum = w_adj.sum().to(torch.float32)
    mod = hip_for(C)
    if mod is not None:
        mod.cma_update_c(C, *_dense(C, y, w_adj, p_c, hs_f.reshape(1), wsum.reshape(1)), float(c1), float(cmu), float(cc))
        return C
    delta_hs = (1.0 - hs_f) * cc * (2.0 - cc)
    scale = 1.0 + c1 * delta_hs - c1 - cmu * wsum
    rank_mu = (y * w_adj.unsqueeze(-1)).T @ y
    rank_one = torch.outer(p_c, p_c)
    C.mul_(scale).add_(rank_one, alpha=c1).add_(rank_mu, alpha=cmu)
    C.copy_(0.5 * (C + C.T))
    return C


def potrf_tile_(A: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In-place lower Cholesky of one SPD panel (n ≤ 128). On GPU this is
    ONE kernel with the panel LDS-resident (ops/hip/cma.hip
    potrf_panel_kernel) — the building block that removes rocSOLVER's
    small-potf2 chain from the blocked factorization
    (algorithms/cmaes.py _blocked_cholesky). `A` may be a strided view
    (a diagonal block of a larger matrix); its upper triangle is left
    untouched. A non-positive pivot at column j sets `info` (a device
    int32 scalar) to j+1 instead of raising — callers check once per
    factorization, not per panel.

    Eager/CPU reference: torch.linalg.cholesky (raises on failure, which
    the CPU callers rely on; it also zeroes the upper triangle, so
    callers must not rely on the upper half either way)."""
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"expected a square panel, got {tuple(A.shape)}")
    mod = hip_for(A)
    if mod is not None:
        if info is None:
            info = torch.zeros(1, dtype=torch.int32, device=A.device)
        mod.potrf_tile(A, info)
        return A
    A.copy_(torch.linalg.cholesky(A))
    return A
