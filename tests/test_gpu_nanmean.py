"""`ops.nanmean_1d` / `_C.nanmean_1d` (the generation's `mean_eval` in one
launch) against `torch.nanmean` on the GPU, bit for bit: `torch.equal`, and
where torch gives NaN (all-NaN input, +inf and -inf together) NaN.

The lengths sit on both sides of everything at which ATen's reduction changes
shape for a contiguous 1-D fp32 input: 128 (16-byte vector loads begin), the
powers of two at which the block widens (width = last_pow2(n) below 128,
last_pow2(n / 4) from there, at most 512), lengths that leave a tail behind
the last whole 4-vector, and 8192, the longest the kernel takes. Views that
start 1, 2 and 3 elements past a 16-byte boundary take ATen's unaligned head.
"""

import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4000, 4096, 8192]
SCALES = [1.0, 1e-3, 1e4]


def _same(got: torch.Tensor, want: torch.Tensor) -> bool:
    if got.dtype != want.dtype or got.shape != want.shape or got.device != want.device:
        return False
    return bool(torch.equal(got, want) or (torch.isnan(got).all() and torch.isnan(want).all()))


def _cases(base: torch.Tensor):
    """(name, vector) for every NaN / inf pattern the issue lists."""
    n = base.numel()
    nan, inf = float("nan"), float("inf")

    def with_values(positions, value):
        x = base.clone()
        x[positions] = value
        return x

    yield "no_nan", base.clone()
    yield "nan_first", with_values([0], nan)
    yield "nan_last", with_values([n - 1], nan)
    yield "nan_middle", with_values([n // 2], nan)
    yield "nan_every_fourth", with_values(list(range(0, n, 4)), nan)
    yield "all_nan", torch.full_like(base, nan)
    yield "plus_inf", with_values([n // 3], inf)
    yield "minus_inf", with_values([n - 1 - n // 3], -inf)
    both = with_values([n // 3], inf)
    both[n - 1 - n // 3] = -inf  # one element when n == 1: then just -inf
    yield "both_inf", both
    mixed = with_values([n // 2], nan)
    mixed[0] = inf
    yield "inf_and_nan", mixed


@gpu
@requires_gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_nanmean_1d_equals_torch(n):
    import evotorch_amd._C as C
    from evotorch_amd import ops

    gen = torch.Generator(device="cpu").manual_seed(1000 + n)
    unit = torch.randn(n, generator=gen)
    for scale in SCALES:
        base = (unit * scale).cuda()
        for name, x in _cases(base):
            want = torch.nanmean(x)
            assert _same(C.nanmean_1d(x), want), (n, scale, name)
            assert _same(ops.nanmean_1d(x), want), (n, scale, name)


@gpu
@requires_gpu
@pytest.mark.parametrize("n", [127, 128, 129, 131, 513, 4000, 8192])
@pytest.mark.parametrize("start", [1, 2, 3])
def test_nanmean_1d_unaligned_view(n, start):
    import evotorch_amd._C as C

    gen = torch.Generator(device="cpu").manual_seed(77 * n + start)
    # values of mixed magnitude: a different order gives different bits
    whole = (torch.randn(n + 4, generator=gen) * torch.logspace(-3, 4, n + 4)[torch.randperm(n + 4, generator=gen)]).cuda()
    x = whole[start : start + n]
    assert x.data_ptr() % 16 == 4 * start and x.is_contiguous()
    assert _same(C.nanmean_1d(x), torch.nanmean(x)), (n, start)
    x = x.clone()
    x[::4] = float("nan")
    y = whole[start : start + n]
    y.copy_(x)
    assert _same(C.nanmean_1d(y), torch.nanmean(y)), (n, start, "nan")


def test_order_matters_for_the_inputs_used():
    """On the CPU: two summation orders of the mixed-magnitude inputs above
    differ in fp32, so equality with torch does pin the order."""
    gen = torch.Generator(device="cpu").manual_seed(77 * 4000 + 1)
    x = torch.randn(4004, generator=gen) * torch.logspace(-3, 4, 4004)[torch.randperm(4004, generator=gen)]
    forward = torch.tensor(0.0)
    for v in x:
        forward = forward + v
    backward = torch.tensor(0.0)
    for v in x.flip(0):
        backward = backward + v
    assert not torch.equal(forward, backward)


@gpu
@requires_gpu
def test_longer_vectors_and_other_inputs_take_torch(monkeypatch):
    import evotorch_amd._C as C
    from evotorch_amd import ops

    assert ops.NANMEAN_1D_MAX_LENGTH == C.nanmean_1d_max_length() == 8192
    x = torch.randn(8193, device="cuda")
    x[5] = float("nan")
    assert _same(ops.nanmean_1d(x), torch.nanmean(x))
    with pytest.raises(RuntimeError, match="nanmean_1d supports"):
        C.nanmean_1d(x)

    calls = []
    real = C.nanmean_1d
    monkeypatch.setattr(C, "nanmean_1d", lambda t: (calls.append(t.numel()), real(t))[1])
    short = x[:4000]
    strided = torch.randn(4000, 2, device="cuda")[:, 0]
    assert _same(ops.nanmean_1d(short), torch.nanmean(short)) and calls == [4000]
    assert _same(ops.nanmean_1d(strided), torch.nanmean(strided))
    assert _same(ops.nanmean_1d(short.double()), torch.nanmean(short.double()))
    assert _same(ops.nanmean_1d(short.cpu()), torch.nanmean(short.cpu()))
    with ops.unfused_generation_tail():
        assert _same(ops.nanmean_1d(short), torch.nanmean(short))
    assert calls == [4000]


@gpu
@requires_gpu
def test_rejected_operands():
    import evotorch_amd._C as C

    good = torch.randn(64, device="cuda")
    with pytest.raises(RuntimeError, match="ROCm tensor"):
        C.nanmean_1d(good.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        C.nanmean_1d(torch.randn(64, 2, device="cuda")[:, 0])
    with pytest.raises(RuntimeError, match="1-D"):
        C.nanmean_1d(torch.randn(8, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="float32"):
        C.nanmean_1d(good.double())
    with pytest.raises(RuntimeError, match="nanmean_1d supports"):
        C.nanmean_1d(torch.empty(0, device="cuda"))


def test_cpu_and_unbuilt_inputs_are_torch():
    from evotorch_amd import ops

    x = torch.tensor([1.0, float("nan"), 3.0])
    assert torch.equal(ops.nanmean_1d(x), torch.nanmean(x))
    assert torch.isnan(ops.nanmean_1d(torch.full((3,), float("nan"))))
