"""`gaussian_clipup_update(raw, scale)` against `gaussian_clipup_update(raw *
scale)`: the kernel's `g = raw * scale` is one rounded fp32 multiply placed
before the first use, which is what the separate `grad * scale` launch hands
over, so velocity, mu and sigma are equal bit for bit (`torch.equal`) over
several steps. Scales 1/4000 and 1/2000 are the flagship's `num_solutions`
and `num_directions` divisors as torch applies them (a multiply by the fp32
reciprocal); a scale of 1 must change nothing against a call without scales.

L = 1 is the smallest, 257 leaves a virtual 256-block with one element, 6409
is the flagship's length (seven passes of the 1024-thread block).
"""

import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

SCALES = {
    "1/4000": float(np.float32(1.0) / np.float32(4000)),
    "1/2000": float(np.float32(1.0) / np.float32(2000)),
    "1": 1.0,
}
BOUNDS = {
    "free": dict(stdev_min=None, stdev_max=None, stdev_max_change=None),
    # max_speed low enough to clip the velocity, every stdev bound in force
    "clip+bounds": dict(stdev_min=0.08, stdev_max=0.6, stdev_max_change=0.2),
}


@functools.lru_cache(maxsize=None)
def _case(length):
    """(mu, sigma, three raw (mu_grad, sigma_grad) pairs), CPU, read-only.
    Raw sums are of the size a popsize-4000 gradient has before division."""
    g = torch.Generator().manual_seed(4241 + length)
    mu = torch.randn(length, generator=g)
    sigma = 0.1 + 0.4 * torch.rand(length, generator=g)
    grads = tuple((300.0 * torch.randn(length, generator=g), 900.0 * torch.randn(length, generator=g)) for _ in range(3))
    return mu, sigma, grads


@gpu
@requires_gpu
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("length", [1, 257, 6409])
def test_scaled_update_equals_update_of_scaled(length, scale, bounds):
    from evotorch_amd import ops

    s = SCALES[scale]
    kwargs = dict(step_size=0.1125, momentum=0.9, sigma_lr=0.1, **BOUNDS[bounds])
    kwargs["max_speed"] = 0.05 if bounds == "clip+bounds" else 1e6
    mu0, sigma0, grads = _case(length)
    mu_a, sigma_a = mu0.cuda(), sigma0.cuda()
    mu_b, sigma_b = mu0.cuda(), sigma0.cuda()
    vel_a = torch.zeros(length, device="cuda")
    vel_b = torch.zeros(length, device="cuda")
    for mu_raw, sigma_raw in grads:
        mu_raw, sigma_raw = mu_raw.cuda(), sigma_raw.cuda()
        mu_a, sigma_a = ops.gaussian_clipup_update(
            mu_a, sigma_a, vel_a, mu_raw, sigma_raw, mu_grad_scale=s, sigma_grad_scale=s, **kwargs
        )
        if scale == "1":  # the call of before this operand existed
            mu_b, sigma_b = ops.gaussian_clipup_update(mu_b, sigma_b, vel_b, mu_raw, sigma_raw, **kwargs)
        else:
            mu_b, sigma_b = ops.gaussian_clipup_update(mu_b, sigma_b, vel_b, mu_raw * s, sigma_raw * s, **kwargs)
        assert torch.equal(vel_a, vel_b)
        assert torch.equal(mu_a, mu_b)
        assert torch.equal(sigma_a, sigma_b)
    assert bool(torch.isfinite(mu_a).all()) and bool(torch.isfinite(sigma_a).all())
    assert not torch.equal(mu_a, mu0.cuda())


@gpu
@requires_gpu
def test_scale_is_the_division_torch_does():
    """`grad / 4000` on the GPU is `grad * fp32(1/4000)`: the premise under
    which the searcher may hand raw sums and a scale to the update."""
    from evotorch_amd.distributions import SeparableGaussian

    raw = (300.0 * torch.randn(6409, generator=torch.Generator().manual_seed(5))).cuda()
    for count in (4000, 2000, 3, 7):
        assert torch.equal(raw / count, raw * SeparableGaussian._count_scale(count))


@gpu
@requires_gpu
def test_mixed_scales_and_unfused_chain():
    """Different scales for mu and sigma, and the chain of launches under
    `unfused_generation_tail()` given the same scales, agree with the kernel."""
    from evotorch_amd import ops

    mu0, sigma0, grads = _case(257)
    kwargs = dict(step_size=0.1125, momentum=0.9, max_speed=0.05, sigma_lr=0.1, stdev_min=0.08, stdev_max=0.6, stdev_max_change=0.2)
    scales = dict(mu_grad_scale=SCALES["1/4000"], sigma_grad_scale=SCALES["1/2000"])
    out = []
    for fused in (True, False):
        mu, sigma, vel = mu0.cuda(), sigma0.cuda(), torch.zeros(257, device="cuda")
        for mu_raw, sigma_raw in grads:
            if fused:
                mu, sigma = ops.gaussian_clipup_update(mu, sigma, vel, mu_raw.cuda(), sigma_raw.cuda(), **scales, **kwargs)
            else:
                with ops.unfused_generation_tail():
                    mu, sigma = ops.gaussian_clipup_update(mu, sigma, vel, mu_raw.cuda(), sigma_raw.cuda(), **scales, **kwargs)
        out.append((mu, sigma, vel))
    for a, b in zip(*out):
        assert torch.equal(a, b)
