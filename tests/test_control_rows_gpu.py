"""imd_residual_scale_rows on the GPU against the CPU expression that is its contract, ``(x.float() * fp32(s)).to(dtype)``: torch.equal
on every scaled row, raw 16-bit equality on the rows at 1.0 and on 64 sentinel elements either side of every segment, whose base sits 16
bytes past an allocation boundary.  Shapes: one vector per row; 16 segments either side of the wave (64), workgroup (256) and chunk (1024
vectors) sizes; the 13 residuals of an 8 x 8 latent at SD1.5 widths; all rows at 1.0 over NaN data; the edge values of both formats."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import control_rows_cases as CC  # noqa: E402


@pytest.fixture(scope="module", params=CC.DTYPES, ids=[n for n, _ in CC.DTYPES])
def dt(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return request.param[1]


def _run(host, rows, scales):
    """host buffers -> (the buffers after the launch, back on the host); the launch sees views 16 bytes into device allocations"""
    from imagdressing_amd import ops
    dev = [(buf.cuda(), first, n) for buf, first, n in host]
    segs = CC.segment_views(dev, rows)
    for s in segs:
        assert s.data_ptr() % 16 == 0 and s.data_ptr() % 32 == 16 and s.is_contiguous()
    before = ops.SCALE_ROWS_COUNTER["launches"]
    ops.residual_scale_rows(segs, torch.tensor(scales, dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    assert ops.SCALE_ROWS_COUNTER["launches"] == before + 1
    return [(buf.cpu(), first, n) for buf, first, n in dev]


def _check(host, got, rows, scales):
    for k, ((hb, first, n), (gb, _, _)) in enumerate(zip(host, got)):
        x, y = hb[first:first + rows * n].view(rows, n), gb[first:first + rows * n].view(rows, n)
        want = CC.expected(x, scales)
        for r, s in enumerate(scales):
            if float(s) == 1.0:
                assert torch.equal(CC.bits(y[r]), CC.bits(x[r])), (k, r, "a row at 1.0 changed")
            else:
                assert torch.equal(y[r], want[r]), (k, r, s, int((CC.bits(y[r]) != CC.bits(want[r])).sum()))
                assert torch.equal(CC.bits(y[r]), CC.bits(want[r])), (k, r, s, "signed zeros")
        assert torch.equal(CC.bits(gb[:first]), CC.bits(hb[:first])), (k, "leading sentinels")
        assert torch.equal(CC.bits(gb[first + rows * n:]), CC.bits(hb[first + rows * n:])), (k, "trailing sentinels")


CASES = {"one vector": (CC.ONE, 2, [0.5, 1.0]),
         "sixteen segments": (CC.SIXTEEN, 3, [0.8, 1.0, 1.3]),
         "8x8 latent residuals": (CC.SD15_8x8, 4, [0.8, 0.0, 0.8, 0.0])}


@pytest.mark.parametrize("case", list(CASES))
def test_scaled_rows_equal_the_cpu_expression(dt, case):
    row_elems, rows, scales = CASES[case]
    host = CC.host_segments(row_elems, rows, dt, seed=len(case))
    _check(host, _run(host, rows, scales), rows, scales)


def test_rows_at_one_are_not_touched_nan_payloads_included(dt):
    rows, row_elems = 8, (8, 8 * 257, 8 * 1025, 64)
    host = CC.host_segments(row_elems, rows, dt, seed=3)
    nan_bits = torch.tensor([0x7FC1, 0x7E01, 0xFFFF, 0x7F81, 0xFC01, 0x7FFF], dtype=torch.int32).to(torch.int16)          # quiet and signalling, both formats
    for buf, first, n in host:
        raw = buf.view(torch.int16)
        for r in range(rows):
            raw[first + r * n:first + r * n + 6] = nan_bits
        assert int(torch.isnan(buf[first:first + 6].float()).sum()) >= 4          # (two of the patterns are numbers in one format, NaNs in the other)
    got = _run(host, rows, [1.0] * rows)
    for (hb, _, _), (gb, _, _) in zip(host, got):
        assert torch.equal(CC.bits(gb), CC.bits(hb))                          # not one byte


def test_edge_values(dt):
    """+-0, the largest finite value (fp16: x 1.3 overflows to inf as on the CPU), fp16 subnormals, scale -1 and 2^-10.  bf16 inputs stay
    inside fp32's normal range (bf16 subnormals are fp32 subnormals: the device's fp32 denormal mode would enter); no NaN in a scaled row"""
    fi = torch.finfo(dt)
    vals = [0.0, -0.0, fi.max, -fi.max, 1.0, -1.0, fi.max / 2, 3.0 * fi.eps, 1.0 + fi.eps, 1.0 - fi.eps / 2, 0.1, 1e-3, 1000.0, -7.0]
    if dt is torch.float16:          # the subnormals and the smallest normal: every product is a normal fp32 number
        vals += [fi.tiny, -fi.tiny, 2.0 ** -24, -2.0 ** -24, 2.0 ** -23 * 3, 2.0 ** -15, 1023 * 2.0 ** -24, 2.0 ** -14 + 2.0 ** -24, 6.0e-8 * 5, 2.0 ** -20]
    else:                            # small and large, but no product below 2^-126
        vals += [2.0 ** -100, -2.0 ** -100, 2.0 ** 100, 3.0e38, 2.0 ** -110, 1e-30, 1e30]
    special = torch.tensor(vals, dtype=torch.float32)
    scales = [1.3, -1.0, 2.0 ** -10, 0.0, 1.0, 0.3]
    rows = len(scales)
    host = CC.host_segments((32, 8 * 33), rows, dt, seed=9, special=special)
    got = _run(host, rows, scales)
    _check(host, got, rows, scales)
    gb, first, n = got[0]
    y = gb[first:first + rows * n].view(rows, n)
    assert not torch.isnan(y.float()).any()
    assert torch.isinf(y[0, 2].float()) and y[0, 2] > 0 and torch.isinf(y[0, 3].float()) and y[0, 3] < 0          # largest finite x 1.3, as on the CPU
    assert y[1, 2].float() == -fi.max and CC.bits(y[3, :2]).tolist() == [0, -32768]          # scale -1; 0 x (+0, -0) keeps the signs
