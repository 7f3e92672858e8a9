"""Hot-op dispatch: hand-written CDNA4 HIP kernels with eager CPU references.

See `evotorch_amd/ops/dispatch.py` for the routing contract and
`evotorch_amd/ops/hip/` for the gfx950 kernel sources.
"""

from .dispatch import (
    GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH,
    affine_from_noise,
    cma_update_c_,
    clipup_step_,
    domination_counts,
    eager_on_gpu,
    es_gradients,
    fused_adam_step_,
    fused_tail_for,
    gaussian_clipup_update,
    hip_available,
    hip_for,
    hip_required,
    load_hip,
    obsnorm_merge_,
    obsnorm_pack_,
    pareto_ranks,
    potrf_tile_,
    sample_gaussian,
    seed_from_generator,
    snes_gradients,
    unfused_generation_tail,
)

__all__ = [
    "GAUSSIAN_CLIPUP_UPDATE_MAX_LENGTH",
    "affine_from_noise",
    "cma_update_c_",
    "clipup_step_",
    "eager_on_gpu",
    "es_gradients",
    "fused_adam_step_",
    "fused_tail_for",
    "gaussian_clipup_update",
    "obsnorm_merge_",
    "obsnorm_pack_",
    "unfused_generation_tail",
    "hip_available",
    "hip_for",
    "hip_required",
    "load_hip",
    "sample_gaussian",
    "seed_from_generator",
    "snes_gradients",
    "pareto_ranks",
    "potrf_tile_",
    "domination_counts",
]
