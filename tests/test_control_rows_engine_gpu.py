"""``ControlNetModel.forward_nhwc(..., scale_rows=)`` on the GPU: SMALL config with a ControlNet, latent 16 x 16, B = 2 (four batch
rows: cond 0, cond 1, uncond 0, uncond 1).  The rows forward -- zero convs at out_scale 1, one imd_residual_scale_rows launch -- against
the folded forward ``conditioning_scale=s_r`` at the same batch, rows r and B + r of every residual.

The bar is derived, not measured: the zero-conv dispatch does not look at ``out_scale`` (tests/test_control_rows_host.py checks it
against the dispatcher), so both forwards hold the same fp32 sums y = W x + b; the folded one stores RNE16(s y), the rows one
RNE16(s RNE16(y)): at most one unit in the last place apart, measured at the larger magnitude, and bit-equal where s is 1 or -- in
bf16 -- a power of two (tests/test_control_rows_host.py asserts both on the CPU expression)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import control_rows_cases as CC  # noqa: E402
from tests.harness import SMALL, build_pair  # noqa: E402

B = 2


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def setup(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.unet import nchw_to_nhwc8
    dt = request.param
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dt)
    lat = torch.cat([g(100, 1, 4, 16, 16), g(101, 1, 4, 16, 16)]).repeat(2, 1, 1, 1)
    ehs = torch.cat([g(110 + r, 1, 77, 64, scale=0.5) for r in range(2 * B)])
    pose = torch.cat([torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(120 + r)) for r in range(B)]).repeat(2, 1, 1, 1)
    inp = dict(x=nchw_to_nhwc8(lat.cuda(), dt), ehs=ehs.cuda().to(dt).contiguous(), pose=nchw_to_nhwc8(pose.cuda(), dt))
    folded = {}

    def fold(s, **kw):
        """the folded forward at conditioning_scale = s: computed once per scale, never modified"""
        key = (s, tuple(sorted((k, v.depth, v.full) for k, v in kw.items())))
        if key not in folded:
            down, mid = p["e_ctrl"].forward_nhwc(inp["x"], 481, inp["ehs"], inp["pose"], s, **kw)
            folded[key] = [d.clone() for d in down] + ([mid.clone()] if mid is not None else [])
        return folded[key]
    return dict(ctrl=p["e_ctrl"], inp=inp, dtype=dt, fold=fold)


def _rows(setup, scales, **kw):
    from imagdressing_amd import ops
    inp = setup["inp"]
    before = ops.SCALE_ROWS_COUNTER["launches"]
    sr = torch.tensor(list(scales) * 2, dtype=torch.float32).cuda()
    down, mid = setup["ctrl"].forward_nhwc(inp["x"], 481, inp["ehs"], inp["pose"], 1.0, scale_rows=sr, **kw)
    assert ops.SCALE_ROWS_COUNTER["launches"] == before + 1                  # ONE launch for all residuals
    return down + ([mid] if mid is not None else [])


@torch.no_grad()
def test_the_residuals_are_fresh_tensors_of_the_forward(setup):
    """what the in-place launch writes is read by nothing else: every residual is its own allocation, distinct from every other and from
    the next forward's"""
    a = _rows(setup, (0.8, 0.4))
    b = _rows(setup, (0.8, 0.4))
    ptrs = [t.untyped_storage().data_ptr() for t in a + b]
    assert len(set(ptrs)) == len(ptrs)
    assert all(t.is_contiguous() and t.storage_offset() == 0 and t.shape[0] == 2 * B for t in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("scales", [(0.8, 0.4), (1.3, 0.05), (0.0, -1.0)], ids=str)
@torch.no_grad()
def test_rows_forward_is_within_one_ulp_of_each_folded_forward(setup, scales):
    rows = _rows(setup, scales)
    worst, differ, total = 0, 0, 0
    for r, s in enumerate(scales):
        folded = setup["fold"](s)
        assert len(folded) == len(rows) == 13
        for k, (a, f) in enumerate(zip(rows, folded)):
            for row in (r, B + r):
                assert torch.isfinite(a[row].float()).all()
                d = CC.ulp_distance(a[row].cpu(), f[row].cpu())
                worst, differ, total = max(worst, int(d.max())), differ + int((d > 0).sum()), total + d.numel()
                assert int(d.max()) <= 1, (k, row, s, int(d.max()))
    print(f"control rows engine {setup['dtype']} scales {scales}: worst {worst} ulp, {differ} of {total} elements differ")
    assert all(float(t.float().abs().max()) > 0 for t in setup["fold"](scales[1]))          # (the zero convs of the test model are not zero)


@torch.no_grad()
def test_powers_of_two_are_bit_equal_in_bf16_and_one_is_always(setup):
    rows = _rows(setup, (0.5, 0.25))
    if setup["dtype"] is torch.bfloat16:
        for r, s in enumerate((0.5, 0.25)):
            for a, f in zip(rows, setup["fold"](s)):
                assert torch.equal(CC.bits(a[r]), CC.bits(f[r])) and torch.equal(CC.bits(a[B + r]), CC.bits(f[B + r]))
    # rows at 1.0 keep the bytes of the conditioning_scale = 1.0 forward, whatever the other request asks for
    rows = _rows(setup, (1.0, 0.3))
    for a, f in zip(rows, setup["fold"](1.0)):
        assert torch.equal(CC.bits(a[0]), CC.bits(f[0])) and torch.equal(CC.bits(a[B]), CC.bits(f[B]))
    for a, f, one in zip(rows, setup["fold"](0.3), setup["fold"](1.0)):
        assert int(CC.ulp_distance(a[1].cpu(), f[1].cpu()).max()) <= 1 and not torch.equal(a[1], one[1])


@pytest.mark.parametrize("depth", [1, 2])
@torch.no_grad()
def test_shallow_deepcache_mode_scales_the_residuals_that_exist(setup, depth):
    from imagdressing_amd.unet import DeepCache
    scales = (0.8, 0.4)

    def cache():
        dc = DeepCache(depth)
        dc.full = True
        setup["ctrl"].forward_nhwc(setup["inp"]["x"], 481, setup["inp"]["ehs"], setup["inp"]["pose"], 1.0, deepcache=dc)
        dc.full = False
        return dc
    rows = _rows(setup, scales, deepcache=cache())
    assert len(rows) == depth                                                # mid is None there; the launch took `depth` segments
    for r, s in enumerate(scales):
        folded = setup["fold"](s, deepcache=cache())
        assert len(folded) == depth
        for a, f in zip(rows, folded):
            for row in (r, B + r):
                assert int(CC.ulp_distance(a[row].cpu(), f[row].cpu()).max()) <= 1


@torch.no_grad()
def test_both_a_scalar_and_rows_is_an_error(setup):
    inp = setup["inp"]
    with pytest.raises(ValueError, match="both given"):
        setup["ctrl"].forward_nhwc(inp["x"], 481, inp["ehs"], inp["pose"], 0.8, scale_rows=torch.ones(2 * B, device="cuda"))
