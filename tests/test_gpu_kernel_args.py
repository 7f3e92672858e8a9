"""Operand checks of the `_C` entry points (ops/hip/check.h).

Every launcher checks every tensor operand before it allocates or launches
anything. `test_rejected` hands each entry point one bad operand and checks
that the error names it and that no output was touched; `test_accepted_*`
makes the matching call with exact sizes and compares it with the eager path.

Every bad operand is harmless even if its check were missing: it is either
LONGER than the kernel reads, a strided view of a larger dense buffer, or of
another dtype with at least as many bytes. Nothing here is short, on another
device, or negative: a regression must show as a failed assertion, never as a
GPU fault.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

SENTINEL = -7.0
# the v6 rollout geometry "linear_base" of test_gpu_rollout_general.py, one member, one step
O, A, R = 32, 8, 8


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


def _full(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")


def _vec(n, dtype=torch.float32):
    return torch.linspace(0.5, 1.5, n, device="cuda").to(dtype)


def _strided(n, dtype=torch.float32):
    """n elements, every second one of a dense buffer of 2n."""
    return _vec(2 * n, dtype)[::2]


# Each case: name -> (operand, or phrase, the error must name; builder). A builder returns
# (call, outputs): `call(C)` makes the rejected call, `outputs` are the tensors
# that must still hold SENTINEL afterwards.


def _sampling_case(entry, length, dtype, bad):
    def build():
        out = _full(4, length, dtype=dtype)
        mu = _vec(length + 4, dtype) if bad == "mu_long" else _vec(length, torch.float32 if bad == "mu_fp32" else dtype)
        sigma = _strided(length, dtype) if bad == "sigma_strided" else _vec(length, dtype)
        if entry == "sample_gaussian":
            return (lambda C: C.sample_gaussian(out, mu, sigma, False, 11)), [out]
        if entry == "sample_gaussian_graphsafe":
            seed_buf = torch.full((1,), 1234, dtype=torch.int64, device="cuda")

            def call(C):
                try:
                    C.sample_gaussian_graphsafe(out, mu, sigma, False, seed_buf)
                finally:
                    assert int(seed_buf) == 1234  # the seed chain did not advance

            return call, [out]
        z = torch.zeros(4 * length, device="cuda")
        return (lambda C: C.affine_from_noise(out, z, mu, sigma, False)), [out]

    return build


def _grad_case(entry, bad):
    def build():
        n, length = (5, 6) if bad == "odd_n" else (4, 6)
        samples = torch.ones(n, length, device="cuda")
        mu = _vec(length)
        sigma = _vec(length + 4) if bad == "sigma_long" else _vec(length)
        weights = _vec(n + 2) if bad == "weights_long" else _vec(n)
        if entry == "snes":
            return (lambda C: C.snes_gradients(samples, mu, sigma, weights)), []
        return (lambda C: C.es_gradients(samples, mu, sigma, weights, entry == "es_symmetric")), []

    return build


def _clipup_case(bad):
    def build():
        velocity = _full(10)
        grad = _vec(12) if bad == "long" else _strided(10)
        return (lambda C: C.clipup_step(velocity, grad, 0.01, 0.15, 0.9)), [velocity]

    return build


def _adam_case(graphsafe, bad):
    def build():
        step_out, m, v = _full(10), _full(10), _full(10)
        grad = _vec(10)
        if bad == "grad":
            grad = _vec(12)
        elif bad == "m":
            m = _full(12)
        else:
            v = _full(12)
        if not graphsafe:
            return (lambda C: C.adam_step(step_out, grad, m, v, 1, 1e-2, 0.9, 0.999, 1e-8)), [step_out, m, v]
        t_buf = torch.zeros(1, dtype=torch.int64, device="cuda")

        def call(C):
            try:
                C.adam_step_graphsafe(step_out, grad, m, v, t_buf, 1e-2, 0.9, 0.999, 1e-8)
            finally:
                assert int(t_buf) == 0  # the step count did not advance

        return call, [step_out, m, v]

    return build


def _cma_case(bad):
    def build():
        d, lam = 5, 3
        Cm = _full(d, d)
        Y = torch.ones(lam, d + 1 if bad == "Y" else d, device="cuda")
        w = _vec(lam + 1 if bad == "w" else lam)
        pc = _vec(d + 1 if bad == "pc" else d)
        hs_f = _vec(2 if bad == "hs_f" else 1)
        wsum = _vec(1, torch.float64 if bad == "wsum" else torch.float32)
        return (lambda C: C.cma_update_c(Cm, Y, w, pc, hs_f, wsum, 0.02, 0.05, 0.1)), [Cm]

    return build


def _mapelites_operands():
    # 2 x 2 x 2: two cells over two features; N = 3
    grid = torch.tensor([[[0.0, 0.5], [0.0, 1.0]], [[0.5, 1.0], [0.0, 1.0]]], device="cuda")
    feats = torch.tensor([[0.1, 0.2], [0.7, 0.3], [0.2, 0.9]], device="cuda")
    utils = torch.tensor([0.3, -1.0, 0.8], device="cuda")
    return grid, feats, utils


def _mapelites_case(bad):
    def build():
        grid, feats, utils = _mapelites_operands()
        if bad == "feats":
            feats = torch.rand(3, 3, device="cuda")
        else:
            utils = _vec(4)
        return (lambda C: C.mapelites_assign(grid, feats, utils)), []

    return build


def _rollout_operands():
    from evotorch_amd.neuroevolution.synthetic_env import SyntheticEnvSpec

    spec = SyntheticEnvSpec(episode_length=1, obs_dim=O, act_dim=A, rank=R, policy_hidden=0, device="cuda")
    g = torch.Generator().manual_seed(2001)
    params = (0.1 * torch.randn(1, spec.solution_length, generator=g)).cuda()
    mean = torch.zeros(O, device="cuda")
    std = torch.ones(O, device="cuda")
    return spec, params, mean, std


def _rollout(C, spec, params, blob, stats):
    return C.rollout_linear(params, blob, stats, O, A, R, 1, spec.alive_bonus, spec.act_cost, 41, 0)


def _rollout_case(bad):
    def build():
        spec, params, mean, std = _rollout_operands()
        blob = spec.env_blob(mean, std, device="cuda")
        assert blob.numel() == (2 * R + A + 4) * O
        stats = _full(2 * O)
        if bad == "env_blob":
            blob = torch.cat([blob, torch.ones(O, device="cuda")])
        else:
            stats = _full(2 * O + 2)
        return (lambda C: _rollout(C, spec, params, blob, stats)), [stats]

    return build


f32, bf16 = torch.float32, torch.bfloat16
REJECTED = {}
for _entry in ("sample_gaussian", "sample_gaussian_graphsafe"):
    for _length in (6, 8):  # generic path, float4 path
        REJECTED[f"{_entry}-L{_length}-mu_long"] = ("mu", _sampling_case(_entry, _length, f32, "mu_long"))
        REJECTED[f"{_entry}-L{_length}-sigma_strided"] = ("sigma", _sampling_case(_entry, _length, f32, "sigma_strided"))
    REJECTED[f"{_entry}-bf16_out-fp32_mu"] = ("mu", _sampling_case(_entry, 6, bf16, "mu_fp32"))
REJECTED["affine_from_noise-mu_long"] = ("mu", _sampling_case("affine_from_noise", 6, f32, "mu_long"))
for _entry in ("es_plain", "es_symmetric", "snes"):
    REJECTED[f"{_entry}-weights_long"] = ("weights", _grad_case(_entry, "weights_long"))
    REJECTED[f"{_entry}-sigma_long"] = ("sigma", _grad_case(_entry, "sigma_long"))
REJECTED["es_symmetric-odd_n"] = ("even popsize", _grad_case("es_symmetric", "odd_n"))
REJECTED["clipup-grad_long"] = ("grad", _clipup_case("long"))
REJECTED["clipup-grad_strided"] = ("grad", _clipup_case("strided"))
for _graphsafe in (False, True):
    for _bad in ("grad", "m", "v"):
        REJECTED[f"adam{'_graphsafe' if _graphsafe else ''}-{_bad}_long"] = (_bad, _adam_case(_graphsafe, _bad))
for _bad in ("Y", "w", "pc", "hs_f", "wsum"):
    REJECTED[f"cma_update_c-{_bad}"] = (_bad, _cma_case(_bad))
REJECTED["mapelites-feats_cols"] = ("feats", _mapelites_case("feats"))
REJECTED["mapelites-utils_long"] = ("utils", _mapelites_case("utils"))
REJECTED["rollout-env_blob_long"] = ("env_blob", _rollout_case("env_blob"))
REJECTED["rollout-obs_stats_long"] = ("obs_stats_out", _rollout_case("obs_stats_out"))


@requires_gpu
@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected(C, case):
    named, build = REJECTED[case]
    call, outputs = build()
    with pytest.raises(RuntimeError) as err:
        call(C)
    # the message names the operand ("mu must have 6 elements, got 10")
    needle = named if " " in named else f"{named} must "
    assert needle in str(err.value), str(err.value)
    torch.cuda.synchronize()
    for out in outputs:
        assert bool((out == SENTINEL).all()), "an output was written before the operand was rejected"


# --------------------------------------------------------------------------
# accepted calls: the same smallest shapes with exact sizes, against the eager
# path at the tolerances of the matching tests in test_gpu_kernels.py
# --------------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("length", [6, 8])
@pytest.mark.parametrize("graphsafe", [False, True])
def test_accepted_sample_gaussian(C, length, graphsafe):
    from evotorch_amd.ops import eager_on_gpu, sample_gaussian
    from evotorch_amd.ops.dispatch import splitmix64

    mu, sigma = _vec(length), _vec(length) + 0.25
    out, ref = _full(4, length), _full(4, length)
    if graphsafe:
        seed_buf = torch.full((1,), 1234, dtype=torch.int64, device="cuda")
        C.sample_gaussian_graphsafe(out, mu, sigma, True, seed_buf)
        assert int(seed_buf) == splitmix64(1234)
    else:
        C.sample_gaussian(out, mu, sigma, True, 1234)
    with eager_on_gpu():
        sample_gaussian(ref, mu, sigma, symmetric=True, seed=1234)
    assert torch.allclose(out, ref, atol=1e-4, rtol=1e-4)  # TestSampleGaussian.test_matches_philox_reference


@requires_gpu
def test_accepted_affine_from_noise(C):
    from evotorch_amd.ops import affine_from_noise, eager_on_gpu

    mu, sigma = _vec(6), _vec(6) + 0.25
    z = torch.randn(4 * 6, generator=torch.Generator().manual_seed(3)).cuda()
    out, ref = _full(4, 6), _full(4, 6)
    C.affine_from_noise(out, z, mu, sigma, False)
    with eager_on_gpu():
        affine_from_noise(ref, z, mu, sigma, symmetric=False)
    # fmaf against multiply-then-add: the fp32 bound of test_kernel_fuzz_random_shapes
    assert torch.allclose(out, ref, atol=1e-5)


@requires_gpu
@pytest.mark.parametrize("entry", ["es_plain", "es_symmetric", "snes"])
def test_accepted_gradients(C, entry):
    from evotorch_amd.ops import eager_on_gpu, es_gradients, snes_gradients

    g = torch.Generator().manual_seed(5)
    mu, sigma, weights = _vec(6), _vec(6) + 0.25, torch.randn(4, generator=g).cuda()
    samples = mu + sigma * torch.randn(4, 6, generator=g).cuda()
    if entry == "snes":
        got = C.snes_gradients(samples, mu, sigma, weights)
        with eager_on_gpu():
            ref = snes_gradients(samples, mu, sigma, weights)
    else:
        got = C.es_gradients(samples, mu, sigma, weights, entry == "es_symmetric")
        with eager_on_gpu():
            ref = es_gradients(samples, mu, sigma, weights, symmetric=entry == "es_symmetric")
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-3)  # TestEsGradients


@requires_gpu
def test_accepted_clipup(C):
    from evotorch_amd.ops import clipup_step_, eager_on_gpu

    velocity = _vec(10) * 0.01
    ref = velocity.clone()
    grad = torch.randn(10, generator=torch.Generator().manual_seed(6)).cuda()
    C.clipup_step(velocity, grad, 0.01, 0.15, 0.9)
    with eager_on_gpu():
        clipup_step_(ref, grad, step_size=0.01, max_speed=0.15, momentum=0.9)
    assert torch.allclose(velocity, ref, rtol=1e-4, atol=1e-6)  # TestOptimizerKernels.test_clipup_matches_eager


@requires_gpu
@pytest.mark.parametrize("graphsafe", [False, True])
def test_accepted_adam(C, graphsafe):
    from evotorch_amd.ops import eager_on_gpu, fused_adam_step_

    grad = torch.randn(10, generator=torch.Generator().manual_seed(7)).cuda()
    out, m, v = _full(10), torch.zeros(10, device="cuda"), torch.zeros(10, device="cuda")
    ref, m_ref, v_ref = _full(10), m.clone(), v.clone()
    if graphsafe:
        t_buf = torch.zeros(1, dtype=torch.int64, device="cuda")
        C.adam_step_graphsafe(out, grad, m, v, t_buf, 1e-2, 0.9, 0.999, 1e-8)
        assert int(t_buf) == 1
    else:
        C.adam_step(out, grad, m, v, 1, 1e-2, 0.9, 0.999, 1e-8)
    with eager_on_gpu():
        fused_adam_step_(ref, grad, m_ref, v_ref, step_count=1, stepsize=1e-2)
    for a, b in ((out, ref), (m, m_ref), (v, v_ref)):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-7)  # TestOptimizerKernels.test_adam_matches_eager


@requires_gpu
def test_accepted_cma_update_c(C):
    from evotorch_amd.ops import cma_update_c_, eager_on_gpu

    d, lam = 5, 3
    g = torch.Generator().manual_seed(8)
    Cm = (torch.eye(d) * 2.0).cuda()
    ref = Cm.clone()
    Y, w, pc = torch.randn(lam, d, generator=g).cuda(), _vec(lam) / lam, torch.randn(d, generator=g).cuda()
    hs_f = torch.ones(1, device="cuda")
    C.cma_update_c(Cm, Y, w, pc, hs_f, w.sum().reshape(1), 0.1, 0.2, 0.3)
    with eager_on_gpu():
        cma_update_c_(ref, Y, w, pc, hs_f[0], c1=0.1, cmu=0.2, cc=0.3)
    assert torch.allclose(Cm, ref, rtol=1e-4, atol=1e-4)  # test_cma_update_c_matches_eager
    assert torch.equal(Cm, Cm.T)


@requires_gpu
def test_accepted_potrf_tile(C):
    B = torch.randn(5, 5, generator=torch.Generator().manual_seed(9)).cuda()
    M = B @ B.T + 5 * torch.eye(5, device="cuda")
    ref = torch.linalg.cholesky(M)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    C.potrf_tile(M, info)
    assert int(info) == 0
    torch.testing.assert_close(torch.tril(M), ref, rtol=3e-5, atol=3e-5)  # test_potrf_tile_matches_torch


@requires_gpu
def test_accepted_mapelites_assign(C):
    grid, feats, utils = _mapelites_operands()
    best, valid = C.mapelites_assign(grid, feats, utils)
    inside = ((feats.unsqueeze(0) >= grid[:, :, 0].unsqueeze(1)) & (feats.unsqueeze(0) <= grid[:, :, 1].unsqueeze(1))).all(-1)
    masked = torch.where(inside, utils.unsqueeze(0), torch.full_like(utils, float("-inf")).unsqueeze(0).expand_as(inside))
    assert valid.tolist() == [True, True] and torch.equal(valid, inside.any(dim=1))
    assert torch.equal(best, masked.argmax(dim=1))  # cell 0 holds rows 0 and 2, cell 1 holds row 1


@requires_gpu
def test_accepted_rollout_linear(C):
    from evotorch_amd.neuroevolution.synthetic_env import rollout_eager
    from evotorch_amd.ops import eager_on_gpu

    spec, params, mean, std = _rollout_operands()
    stats = torch.zeros(2 * O, device="cuda")
    fit = _rollout(C, spec, params, spec.env_blob(mean, std, device="cuda"), stats)
    with eager_on_gpu():
        efit, (_, esum, esumsq) = rollout_eager(spec, params, mean, std, init_seed=41)
    # TestRollout.test_matches_eager_reference
    assert torch.allclose(fit, efit, rtol=2e-2, atol=2e-2), (fit, efit)
    assert torch.allclose(stats[:O], esum, rtol=5e-2, atol=5e-1)
    assert torch.allclose(stats[O:], esumsq, rtol=5e-2, atol=5e-1)
