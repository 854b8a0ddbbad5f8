"""``imd_lora_expand_rows`` on the device, both element types.

* exact family (tests/lora_rows_cases.py): ``torch.equal`` with the float64 expectation, pass-through columns included;
* a sentinel guard: ``out_ld = C + T + 24`` and ``x_ld = C + 8`` with sentinel-filled slack that must survive;
* Gaussian operands at the same shapes with scales that include 0 and negative values: the tail within ONE unit in the last place of
  the element type of the float64 value (fp32 accumulation over K <= 1280 errs far below a 16-bit half-ulp, so only the final
  rounding may pick the neighbour), the pass-through ``torch.equal``, zero-scale rows all zero."""
import numpy as np
import pytest
import torch

from tests import lora_rows_cases as LC

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = lambda s: "C%d_T%d_E%dx%d" % s if isinstance(s, tuple) else str(s).split(".")[-1]      # noqa: E731


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", LC.SHAPES, ids=IDS)
def test_exact_family(shape, dtype):
    from imagdressing_amd import ops
    C, T, E, rpe = shape
    x, down, scale = LC.exact_operands(C, T, E, rpe)
    want = _dev(LC.expected(x, down, scale, rpe), dtype)
    xd = _dev(x, dtype)
    out = ops.lora_expand_rows(xd, _dev(down, dtype), _dev(scale, torch.float32), rpe)
    assert out.shape == (E * rpe, C + T) and out.dtype == dtype
    assert torch.equal(out[:, :C], xd)
    bad = (out != want).nonzero()
    assert torch.equal(out, want), f"{bad.shape[0]} elements differ, first at {bad[:4].tolist()}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_slack_of_strided_rows_survives(dtype):
    """x rows 8 elements apart from each other's end, out rows with 24 elements of slack: the kernel reads x through x_ld and writes
    C + T elements of a row, not one byte more"""
    from imagdressing_amd import ops
    C, T, E, rpe = 80, 16, 2, 72
    M = E * rpe
    x, down, scale = LC.exact_operands(C, T, E, rpe, seed=1)
    xbuf = torch.full((M, C + 8), 777.0, dtype=dtype, device="cuda")
    xbuf[:, :C] = _dev(x, dtype)
    obuf = torch.full((M + 2, C + T + 24), -999.0, dtype=dtype, device="cuda")      # a guard row on either side as well
    before = obuf.clone()
    out = ops.lora_expand_rows(xbuf[:, :C], _dev(down, dtype), _dev(scale, torch.float32), rpe, out=obuf[1:M + 1])
    assert out.data_ptr() == obuf[1].data_ptr()
    assert torch.equal(obuf[1:M + 1, :C + T], _dev(LC.expected(x, down, scale, rpe), dtype))
    assert torch.equal(obuf[1:M + 1, C + T:], before[1:M + 1, C + T:])
    assert torch.equal(obuf[0], before[0]) and torch.equal(obuf[M + 1], before[M + 1])
    assert torch.equal(xbuf[:, C:], torch.full((M, 8), 777.0, dtype=dtype, device="cuda"))


def _ulp(v, dtype):
    """spacing of the element type at |v| (float64 tensor), subnormal spacing below the smallest normal"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - mant)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", LC.SHAPES, ids=IDS)
def test_gaussian_operands_within_one_ulp(shape, dtype):
    from imagdressing_amd import ops
    C, T, E, rpe = shape
    g = torch.Generator(device="cpu").manual_seed(C * 31 + T)
    # Gaussians around 1 (sigma 1/4), every `down` row with a sign and a magnitude 1 .. 16 / C of its own: the terms of one sum share
    # a sign, so no sum cancels.  That is what the one-ulp bound rests on: the fp32 accumulation errs by at most K 2^-24 of the sum of
    # the terms' magnitudes (1280 2^-24 = 2^-13.7, a sixth of an fp16 ulp), which is "far below a half-ulp" of the RESULT only where
    # the result is of that magnitude.  With zero-mean operands some of the 10^5 sums cancel to 10^-4 of it, where an fp16 ulp is
    # smaller than the fp32 rounding of the partial sums (measured with them at C = 320, T = 384: 1.73 fp16 ulp at such an element).
    xd = (1.0 + 0.25 * torch.randn(E * rpe, C, generator=g)).to("cuda").to(dtype)
    sign = torch.where(torch.rand(T, 1, generator=g) < 0.5, -1.0, 1.0)
    mag = torch.pow(2.0, torch.randint(0, 5, (T, 1), generator=g).float()) / C
    dd = (sign * mag * (1.0 + 0.25 * torch.randn(T, C, generator=g))).to("cuda").to(dtype)
    scale = torch.tensor([(0.0, -0.75, 1.3, 0.4, -2.0, 1.0)[e % 6] for e in range(E)], dtype=torch.float32, device="cuda")
    out = ops.lora_expand_rows(xd, dd, scale, rpe)
    assert torch.equal(out[:, :C], xd)
    ref = scale.double().repeat_interleave(rpe)[:, None] * (xd.double() @ dd.double().T)
    err = (out[:, C:].double() - ref).abs()
    ulp = _ulp(ref, dtype)
    worst = (err / ulp).max().item()
    assert worst <= 1.0, f"worst error {worst:.3f} ulp"
    zero_rows = (scale == 0).repeat_interleave(rpe)
    assert zero_rows.any() and bool((out[zero_rows][:, C:] == 0).all())
    assert bool((out[~zero_rows][:, C:] != 0).any())
