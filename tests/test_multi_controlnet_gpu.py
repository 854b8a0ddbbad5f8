"""imd_residual_mix_rows on the GPU against the CPU expression that is its contract (tests/multi_controlnet_cases.py: the chain of
``x.float() * fp32(s)`` and ``+`` in source order, a source at 0 skipped): torch.equal and raw 16-bit equality of every dst segment, raw
equality of 64 sentinel elements either side of every dst and source segment and of every source that is not the destination.  Shapes:
one vector per row; 16 segments either side of the wave, workgroup and chunk sizes; the 13 residuals of an 8 x 8 latent; one segment
(a DeepCache call of depth 1); rows 1, 3, 4; 1..4 sources; every scale pattern; dst separate, on source 0 and on the last source.  The
data carries the crafted block under which a contracted (FMA) or reordered sum differs (test_multi_controlnet_inputs.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import multi_controlnet_cases as M  # noqa: E402
from tests.control_rows_cases import ONE, SD15_8x8, SIXTEEN, bits, host_segments, segment_views  # noqa: E402

SHAPES = {"one vector": ONE, "sixteen segments": SIXTEEN, "8x8 latent residuals": SD15_8x8, "single segment": (8 * 320,)}
ALIAS = ("separate", "source 0", "last source")


@pytest.fixture(scope="module", params=M.DTYPES, ids=[n for n, _ in M.DTYPES])
def dt(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return request.param[1]


def _launch(host_src, host_dst, rows, scales, alias):
    """host buffers -> (source buffers, dst buffers) after the launch, back on the host; dst = the buffers of a source when aliased"""
    from imagdressing_amd import ops
    dev_src = [[(buf.cuda(), first, n) for buf, first, n in src] for src in host_src]
    if alias == "separate":
        dev_dst = [(buf.cuda(), first, n) for buf, first, n in host_dst]
    else:
        dev_dst = dev_src[0 if alias == "source 0" else -1]
    srcs, dst = [segment_views(d, rows) for d in dev_src], segment_views(dev_dst, rows)
    for s in dst + [t for src in srcs for t in src]:
        assert s.data_ptr() % 32 == 16 and s.is_contiguous()          # 16 bytes past an allocation boundary, no more
    before = ops.MIX_ROWS_COUNTER["launches"]
    out = ops.residual_mix_rows(srcs, torch.tensor(scales, dtype=torch.float32).cuda(), out=dst)
    torch.cuda.synchronize()
    assert ops.MIX_ROWS_COUNTER["launches"] == before + 1 and all(o is d for o, d in zip(out, dst))
    back = lambda bufs: [(buf.cpu(), first, n) for buf, first, n in bufs]          # noqa: E731
    return [back(d) for d in dev_src], back(dev_dst)


def _check(host_src, host_dst, got_src, got_dst, rows, scales, alias, tag):
    K = len(host_src)
    views = [segment_views(src, rows) for src in host_src]
    target = None if alias == "separate" else (0 if alias == "source 0" else K - 1)
    for j, (gb, first, n) in enumerate(got_dst):
        want = M.mix([views[k][j] for k in range(K)], scales)
        y = gb[first:first + rows * n].view(rows, n)
        assert torch.equal(y, want), (tag, j, int((bits(y) != bits(want)).sum()))
        assert torch.equal(bits(y), bits(want)), (tag, j, "signed zeros")
        before = (host_dst if target is None else host_src[target])[j][0]
        assert torch.equal(bits(gb[:first]), bits(before[:first])), (tag, j, "leading sentinels of dst")
        assert torch.equal(bits(gb[first + rows * n:]), bits(before[first + rows * n:])), (tag, j, "trailing sentinels of dst")
    for k in range(K):
        if k == target:
            continue
        for j, ((hb, _, _), (gb, _, _)) in enumerate(zip(host_src[k], got_src[k])):
            assert torch.equal(bits(gb), bits(hb)), (tag, k, j, "a source that is not the destination changed")


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("rows", [1, 3, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mix_equals_the_cpu_expression(dt, shape, rows, K):
    row_elems = SHAPES[shape]
    host_src = M.source_buffers(row_elems, rows, dt, K, seed=len(shape) + rows)
    host_dst = host_segments(row_elems, rows, dt, seed=999)          # (Gaussian too: a dst that is not written shows)
    for name, scales in M.scale_patterns(K, rows):
        for alias in ALIAS:
            if K == 1 and alias == "last source":
                continue
            got_src, got_dst = _launch(host_src, host_dst, rows, scales, alias)
            _check(host_src, host_dst, got_src, got_dst, rows, scales, alias, (name, alias))
            if name == "all_zero":
                assert all(not bits(gb[first:first + rows * n]).any() for gb, first, n in got_dst), (name, alias, "+0")
            if name.startswith("one"):
                k = int(name[3:])
                for (gb, first, n), (hb, _, _) in zip(got_dst, host_src[k]):
                    assert torch.equal(bits(gb[first:first + rows * n]), bits(hb[first:first + rows * n])), (name, alias, "the source's bits")


def test_a_gated_source_is_not_read(dt):
    """NaN and Inf all over the gated source: the result is that of the open sources alone, finite"""
    rows, K = 3, 3
    host_src = M.source_buffers(SIXTEEN, rows, dt, K, seed=5)
    for buf, first, n in host_src[1]:
        buf[first:first + rows * n:2] = float("nan")
        buf[first + 1:first + rows * n:2] = float("inf")
    scales = [[0.7, 0.7, 0.0], [0.0, 0.0, 0.0], [-0.45, 0.0, 0.9]]
    host_dst = host_segments(SIXTEEN, rows, dt, seed=999)
    got_src, got_dst = _launch(host_src, host_dst, rows, scales, "separate")
    _check(host_src, host_dst, got_src, got_dst, rows, scales, "separate", "gated")
    assert all(bool(torch.isfinite(gb[first:first + rows * n].float()).all()) for gb, first, n in got_dst)


def test_more_chunks_than_the_grid(dt):
    """one segment of 3 rows x 700 chunks, K = 2: 2100 chunks on 2048 workgroups -- the stride loop runs twice for the first 52"""
    rows, n = 3, 700 * 1024 * 8
    g = torch.Generator().manual_seed(11)
    srcs = [(torch.randn(rows, n, generator=g) * 2.0).to(dt) for _ in range(2)]
    scales = [[0.7, 0.0, -0.45], [1.3, 0.9, 0.0]]
    from imagdressing_amd import ops
    dev = [[s.cuda()] for s in srcs]
    out = ops.residual_mix_rows(dev, torch.tensor(scales, dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    want = M.mix(srcs, scales)
    assert torch.equal(bits(out[0].cpu()), bits(want))
    assert torch.equal(bits(dev[0][0].cpu()), bits(srcs[0])) and torch.equal(bits(dev[1][0].cpu()), bits(srcs[1]))
    got = ops.residual_mix_rows(dev, torch.tensor(scales, dtype=torch.float32).cuda(), out=dev[1])          # in place on the last source
    torch.cuda.synchronize()
    assert got[0] is dev[1][0] and torch.equal(bits(dev[1][0].cpu()), bits(want)) and torch.equal(bits(dev[0][0].cpu()), bits(srcs[0]))


def test_an_overlap_that_is_not_in_place_is_refused(dt):
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    buf = torch.zeros(4 * 64 + 8, dtype=dt, device="cuda")
    a, shifted = buf[:4 * 64].view(4, 64), buf[8:].view(4, 64)
    b = torch.ones(4, 64, dtype=dt, device="cuda")
    before = ops.MIX_ROWS_COUNTER["launches"]
    with pytest.raises(ImdError, match=r"dst\[0\] overlaps src\[0\]\[0\]"):
        ops.residual_mix_rows([[a], [b]], torch.ones(2, 4, device="cuda"), out=[shifted])
    assert ops.MIX_ROWS_COUNTER["launches"] == before and not buf.any()
