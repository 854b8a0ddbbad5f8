"""imd_image_mask_filter on the GPU against Pillow, byte for byte (``torch.equal``): blur alone, the window maximum alone, both; the
LDS form and the one-launch-per-pass form; a batch with row and image strides inside a sentinel-filled buffer; in place; the bounds
against numpy's non-zero box; the input left untouched; every refusal without a launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mask_filter_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops
    ops.ensure_device(torch.device("cuda"))
    return torch.device("cuda")


def run(a, k=0, radius=0.0, **kw):
    from imagdressing_amd import ops
    from imagdressing_amd.image import gaussian_box
    src = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    before = src.clone()
    out = ops.image_mask_filter(src, k, gaussian_box(radius) if radius > 0 else None, **kw)
    assert torch.equal(src, before)                                         # the input is left untouched (out is not src)
    return out


def expected(hw, k, radius):
    """Pillow's result for ``MC.stack(hw)`` as a tensor (a copy: the shared array stays read-only)"""
    return torch.from_numpy(MC.pillow_stack(hw, k, radius).copy())


def ids(hw):
    return f"{hw[0]}x{hw[1]}"


@pytest.mark.parametrize("hw", MC.SIZES, ids=ids)
def test_blur_alone(dev, hw):
    for radius in MC.RADII:
        got = run(MC.stack(hw), 0, radius)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), expected(hw, 0, radius)), (hw, radius)


@pytest.mark.parametrize("hw", MC.SIZES, ids=ids)
def test_dilate_alone(dev, hw):
    for k in MC.DILATES:
        assert torch.equal(run(MC.stack(hw), k, 0.0).cpu(), expected(hw, k, 0.0)), (hw, k)


BOTH = [(1, 0.3), (3, 4), (20, 7.25), (3, 33), (1, 100)]


@pytest.mark.parametrize("hw", MC.SIZES, ids=ids)
def test_both(dev, hw):
    for k, radius in BOTH:
        assert torch.equal(run(MC.stack(hw), k, radius).cpu(), expected(hw, k, radius)), (hw, k, radius)


@pytest.mark.parametrize("hw", [(1, 1), (9, 1), (37, 53), (64, 80)], ids=ids)
def test_one_launch_per_pass_form(dev, hw):
    """the form of lines longer than IMD_IMG_MASK_LINE_MAX, taken here by flag: the same bytes"""
    for k, radius in ((0, 0.3), (0, 4), (0, 33), (3, 0.0), (3, 4), (20, 100), (0, 0.0)):
        got = run(MC.stack(hw), k, radius, _force_global=True)
        assert torch.equal(got.cpu(), expected(hw, k, radius)), (hw, k, radius)


def test_large(dev):
    hw, radius, k = MC.LARGE
    a = MC.images(hw)[0][1]
    want = torch.from_numpy(MC.pillow_filter(a, k, radius))
    got, bounds = run(a[None], k, radius, bounds=True)
    assert torch.equal(got[0].cpu(), want)
    assert tuple(bounds[0].tolist()) == MC.nonzero_box(want.numpy())
    rect = MC.images(hw)[1][1]
    got, bounds = run(rect[None], k, radius, bounds=True)
    want = MC.pillow_filter(rect, k, radius)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want))
    box = MC.nonzero_box(want)
    assert tuple(bounds[0].tolist()) == box and 0 < box[0] and box[2] < hw[1] - 1       # a box inside the image


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "per_pass"])
@pytest.mark.parametrize("hw", [(37, 53), (64, 80), (5, 3)], ids=ids)
def test_batch_with_strides_and_sentinels(dev, hw, force_global):
    """B = 3, row stride W + 5, image stride (H + 3) rows, source and output both strided views of sentinel-filled buffers: the
    filtered masks equal Pillow's, the padding of the output keeps the sentinel, the source buffer is unchanged"""
    from imagdressing_amd import ops
    from imagdressing_amd.image import gaussian_box
    H, W = hw
    buf, masks = MC.strided_batch(hw, seed=11)
    for k, radius in ((0, 4), (3, 0.0), (3, 7.25), (1, 33)):
        src_buf = torch.from_numpy(buf).cuda()
        out_buf = torch.full_like(src_buf, MC.SENTINEL)
        src, out = src_buf[:, :H, :W], out_buf[:, :H, :W]
        assert src.stride() == ((H + 3) * (W + 5), W + 5, 1)
        got = ops.image_mask_filter(src, k, gaussian_box(radius) if radius > 0 else None, out=out, _force_global=force_global)
        assert got.data_ptr() == out.data_ptr()
        want = np.stack([MC.pillow_filter(m, k, radius) for m in masks])
        assert torch.equal(out.cpu(), torch.from_numpy(want)), (hw, k, radius)
        pad = np.ones(buf.shape, bool)
        pad[:, :H, :W] = False
        assert (out_buf.cpu().numpy()[pad] == MC.SENTINEL).all()
        assert torch.equal(src_buf.cpu(), torch.from_numpy(buf))
        # in place: out is src
        again = ops.image_mask_filter(src, k, gaussian_box(radius) if radius > 0 else None, out=src, _force_global=force_global)
        assert again.data_ptr() == src.data_ptr() and torch.equal(src.cpu(), torch.from_numpy(want))
        assert (src_buf.cpu().numpy()[pad] == MC.SENTINEL).all()


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "per_pass"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 9), (5, 3), (37, 53), (200, 150)], ids=ids)
def test_bounds(dev, hw, force_global):
    names = [n for n, _ in MC.images(hw)]
    for k, radius in ((0, 0.0), (0, 1), (3, 0.0), (1, 2), (3, 4)):
        got, bounds = run(MC.stack(hw), k, radius, bounds=True, _force_global=force_global)
        want = MC.pillow_stack(hw, k, radius)
        assert torch.equal(got.cpu(), expected(hw, k, radius))
        assert bounds.dtype == torch.int32 and bounds.shape == (len(names), 4)
        assert [tuple(b) for b in bounds.tolist()] == [MC.nonzero_box(w) for w in want], (hw, k, radius)
        assert tuple(bounds[names.index("zeros")].tolist()) == (hw[1], hw[0], -1, -1)          # the all-zero sentinel


def test_launch_counts(dev):
    from imagdressing_amd import ops
    a = MC.stack((37, 53))

    def launches(*args, **kw):
        before = ops.IMAGE_IO_COUNTER["mask_filter_launches"]
        run(a, *args, **kw)
        return ops.IMAGE_IO_COUNTER["mask_filter_launches"] - before
    assert launches(3, 33) == 3 and launches(0, 100) == 2 and launches(20, 0.0) == 2 and launches(3, 4, bounds=True) == 4


def test_device_processor_and_mask_processor(dev):
    from PIL import Image, ImageFilter
    from imagdressing_amd.image import DeviceImageProcessor, MaskProcessor, crop_region_of_bounds, get_crop_region
    proc = DeviceImageProcessor("cuda", torch.float16)
    a = MC.images((200, 150))[1][1]
    rgb = np.stack([a, a // 2, a // 3], -1)
    for m in (Image.fromarray(a), Image.fromarray(rgb), a):
        pil = m if hasattr(m, "convert") else Image.fromarray(m)
        want = pil.convert("L").filter(ImageFilter.MaxFilter(7)).filter(ImageFilter.GaussianBlur(4))
        got, bounds = proc.mask_filter(m, dilate=3, blur=4.0, bounds=True)
        assert got.shape == (1, 200, 150, 1) and torch.equal(got[0, ..., 0].cpu(), torch.from_numpy(np.array(want)))
        assert crop_region_of_bounds(bounds[0].tolist(), 150, 200, 128, 128, 8) == get_crop_region(want, 128, 128, 8)
    up = torch.from_numpy(a).cuda()
    blurred = MaskProcessor(lambda: proc).blur(up, blur_factor=33)
    assert blurred.shape == up.shape and torch.equal(blurred.cpu(), torch.from_numpy(MC.pillow_filter(a, 0, 33)))
    assert torch.equal(MaskProcessor().blur(up[None, ..., None]).cpu()[0, ..., 0], torch.from_numpy(MC.pillow_filter(a, 0, 4)))
    with pytest.raises(ValueError):
        proc.mask_filter(a, dilate=-1)


def test_refusals_leave_the_output_alone(dev):
    """every refusal, with real buffers: an error by name, and not a byte of the output written"""
    from imagdressing_amd import _lib
    from tests.test_mask_filter_inputs import launchable_block, refusals
    lib = _lib.load()
    src = torch.from_numpy(MC.stack((37, 53))[:2].copy()).cuda()
    out = torch.full((2, 37, 53), MC.SENTINEL, dtype=torch.uint8, device="cuda")
    tmp = torch.full((2, 37, 53), MC.SENTINEL, dtype=torch.uint8, device="cuda")
    bounds = torch.full((2, 4), 77, dtype=torch.int32, device="cuda")
    for over, word in refusals():
        p = launchable_block()
        p.src, p.out, p.tmp, p.bounds = src.data_ptr(), out.data_ptr(), tmp.data_ptr(), bounds.data_ptr()
        for k, v in over.items():
            setattr(p, k, p.out if (k == "tmp" and v is not None) else v)
        assert lib.imd_image_mask_filter(ctypes.byref(p), None) != 0
        err = lib.imd_last_error()
        assert err.startswith(b"image_mask_filter:") and word in err and b"launch failed" not in err, err
    torch.cuda.synchronize()
    assert (out == MC.SENTINEL).all() and (tmp == MC.SENTINEL).all() and (bounds == 77).all()
