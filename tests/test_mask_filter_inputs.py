"""mask_dilate / mask_blur without a GPU: the numpy restatement (``blur_reference``, ``dilate_reference``, ``gaussian_box``) against
Pillow itself on every shared case; that each plausible mistake changes at least one byte of at least one case (so the GPU comparison
can see it); ``mask_filter_host`` against the chained Pillow call; the argument errors of the pipeline; the C ABI of
``imd_image_mask_filter`` -- declared, bound, ``struct_bytes`` checked, every refusal by name before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from imagdressing_amd.image import (blur_reference, crop_region_of_bounds, dilate_reference, gaussian_box, get_crop_region, mask_filter_host,
                                    mask_filter_values)
from tests import mask_filter_cases as MC
from tests.test_abi import declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against Pillow ----
@pytest.mark.parametrize("hw", MC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_reference_equals_pillow(hw):
    for radius in MC.RADII:
        got = blur_reference(MC.stack(hw), radius)
        assert got.dtype == np.uint8 and np.array_equal(got, MC.pillow_stack(hw, 0, radius)), (hw, radius)
    assert np.array_equal(blur_reference(MC.stack(hw), 0.0), MC.stack(hw))


@pytest.mark.parametrize("hw", MC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dilate_reference_equals_pillow(hw):
    for k in MC.DILATES:
        assert np.array_equal(dilate_reference(MC.stack(hw), k), MC.pillow_stack(hw, k, 0.0)), (hw, k)


@pytest.mark.parametrize("hw", [(37, 53), (5, 3), (200, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_steps_equal_pillow(hw):
    for k, radius in ((1, 0.5), (3, 4), (20, 7.25), (3, 33)):
        assert np.array_equal(blur_reference(dilate_reference(MC.stack(hw), k), radius), MC.pillow_stack(hw, k, radius)), (hw, k, radius)


def test_large_case_equals_pillow():
    hw, radius, k = MC.LARGE
    a = MC.images(hw)[0][1]
    assert np.array_equal(blur_reference(dilate_reference(a, k), radius), MC.pillow_filter(a, k, radius))


def test_all_255_stays_and_the_pixel_places_the_window():
    for hw in MC.SIZES:
        names = [n for n, _ in MC.images(hw)]
        for radius in MC.RADII:
            out = MC.pillow_stack(hw, 0, radius)
            assert (out[names.index("ones")] == 255).all() and not out[names.index("zeros")].any()
    # a 255 pixel in the centre of 37 x 53 under k = 3 becomes the 7 x 7 block around it
    out = MC.pillow_stack((37, 53), 3, 0.0)[[n for n, _ in MC.images((37, 53))].index("centre")]
    assert MC.nonzero_box(out) == (26 - 3, 18 - 3, 26 + 3, 18 + 3) and out.sum() == 49 * 255


def test_gaussian_box_integers():
    for radius in MC.RADII:
        r, ww, fw = gaussian_box(radius)
        assert r >= 0 and 0 < ww <= 1 << 24 and fw >= 0
        assert (2 * r + 1) * ww + 2 * fw in ((1 << 24), (1 << 24) - 1)          # what the library checks
    assert gaussian_box(0.3) != MC.box_in_double(0.3)                           # the float32 detail is load-bearing
    assert gaussian_box(33)[0] == 32 and gaussian_box(4)[0] == 3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_box(bad)


# ---- sensitivity: the cases can see each mistake ----
MISTAKES = {
    "box radius in double": lambda a, radius: MC.variant_blur(a, radius, box=MC.box_in_double(radius)),
    "zero padding": lambda a, radius: MC.variant_blur(a, radius, pad="zero"),
    "fw dropped": lambda a, radius: MC.variant_blur(a, radius, use_fw=False),
    "no rounding term": lambda a, radius: MC.variant_blur(a, radius, rounding=0),
    "window shifted": lambda a, radius: MC.variant_blur(a, radius, shift=1),
    "two passes": lambda a, radius: MC.variant_blur(a, radius, passes=2),
    "columns first": lambda a, radius: MC.variant_blur(a, radius, columns_first=True),
}
SENS_RADII = [0.3, 0.5, 1, 1.5, 2, 4, 7.25, 16]          # (the direct windowed sum of the variants is O(r): the larger radii add nothing)


def test_the_variant_tool_without_a_mistake_is_pillow():
    for hw in ((37, 53), (5, 3), (1, 9)):
        for radius in SENS_RADII:
            assert np.array_equal(MC.variant_blur(MC.stack(hw), radius), MC.pillow_stack(hw, 0, radius)), (hw, radius)


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_sensitivity(mistake):
    seen = [(hw, radius) for hw in ((37, 53), (64, 80), (5, 3)) for radius in SENS_RADII
            if not np.array_equal(MISTAKES[mistake](MC.stack(hw), radius), MC.pillow_stack(hw, 0, radius))]
    assert seen, f"no listed case changes under: {mistake}"


def test_dilate_sensitivity():
    """a window one wider, one narrower, or zero-padded... the maximum's mistakes: k off by one changes the centre-pixel case"""
    hw = (37, 53)
    for k in (1, 3, 20):
        assert not np.array_equal(dilate_reference(MC.stack(hw), k + 1), MC.pillow_stack(hw, k, 0.0))
        assert not np.array_equal(dilate_reference(MC.stack(hw), k - 1), MC.pillow_stack(hw, k, 0.0))


# ---- the host route ----
def test_mask_filter_host_is_the_chained_pillow_call():
    from PIL import Image, ImageFilter
    a = MC.images((64, 80))[0][1]
    rgb = np.random.default_rng(3).integers(0, 256, size=(64, 80, 3), dtype=np.uint8)
    for m in (Image.fromarray(a), Image.fromarray(rgb), Image.fromarray(a > 127), a, rgb):
        for k, b in ((0, 0.0), (3, 0.0), (0, 4.0), (3, 4.0), (20, 0.3)):
            pil = m if hasattr(m, "convert") else Image.fromarray(m)
            want = pil.convert("L")
            if k:
                want = want.filter(ImageFilter.MaxFilter(2 * k + 1))
            if b:
                want = want.filter(ImageFilter.GaussianBlur(b))
            got = mask_filter_host(m, k, b)
            assert got.mode == "L" and got.size == want.size and got.tobytes() == want.tobytes()


def test_mask_processor_blur_on_the_host():
    from PIL import Image, ImageFilter
    from imagdressing_amd.image import MaskProcessor
    m = Image.fromarray(MC.images((64, 80))[1][1])
    assert MaskProcessor().blur(m, blur_factor=33).tobytes() == m.filter(ImageFilter.GaussianBlur(33)).tobytes()
    assert MaskProcessor().blur(m).tobytes() == m.filter(ImageFilter.GaussianBlur(4)).tobytes()
    with pytest.raises(TypeError):
        MaskProcessor().blur(torch.zeros(4, 4, dtype=torch.uint8))           # a host tensor: not an uploaded mask


def test_crop_region_of_bounds_is_get_crop_region():
    for hw in ((37, 53), (200, 150), (64, 80)):
        for k, radius in ((0, 0.0), (3, 4), (8, 33)):
            for a in MC.pillow_stack(hw, k, radius):
                box = MC.nonzero_box(a)
                if box[2] < 0:
                    with pytest.raises(ValueError, match="all zero"):
                        crop_region_of_bounds(box, hw[1], hw[0], 128, 96, 8)
                    with pytest.raises(ValueError, match="all zero"):
                        get_crop_region(a, 128, 96, 8)
                else:
                    assert crop_region_of_bounds(box, hw[1], hw[0], 128, 96, 8) == get_crop_region(a, 128, 96, 8)


# ---- the argument errors of the pipeline ----
def test_values_are_checked():
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import _mask_filter_requests
    assert _mask_filter_requests(0, 0.0, 3) is None and _mask_filter_requests([0, 0], [0.0, 0], 2) is None
    assert _mask_filter_requests(2, 0.0, 2) == [(2, 0.0)] * 2
    assert _mask_filter_requests([1, 0], 4, 2) == [(1, 4.0), (0, 4.0)]
    for k, b in ((-1, 0.0), (0, -0.5), (0, float("nan")), (0, float("inf")), (1.5, 0.0), ([1, -2], 0.0), (0, [1.0, float("inf")]), (True, 0.0)):
        with pytest.raises(ValueError):
            _mask_filter_requests(k, b, 2)
    for k, b in (([1, 2, 3], 0.0), (0, [1.0]), ([], 2.0)):
        with pytest.raises(ValueError, match="entries for 2 requests"):
            _mask_filter_requests(k, b, 2)
    assert mask_filter_values(np.int64(3), np.float32(2.5)) == (3, 2.5)


def _bare_pipe():
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    pipe = IMAGDressing_v1.__new__(IMAGDressing_v1)
    pipe.scheduler = None
    return pipe


def _call(pipe, **kw):
    base = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=3,
                guidance_scale=5.0)
    base.update(kw)
    return pipe(**base)


def test_call_errors_precede_any_work():
    """the checks of mask_dilate / mask_blur come before the first engine is touched: a pipeline without engines raises them"""
    from PIL import Image
    pipe = _bare_pipe()
    m = Image.fromarray(MC.images((64, 80))[1][1])
    with pytest.raises(ValueError, match="mask_blur"):
        _call(pipe, mask_image=m, mask_blur=-1.0)
    with pytest.raises(ValueError, match="mask_blur"):
        _call(pipe, mask_image=m, mask_blur=float("nan"))
    with pytest.raises(ValueError, match="mask_dilate"):
        _call(pipe, mask_image=m, mask_dilate=-3)
    with pytest.raises(ValueError, match="entries for 1 requests"):
        _call(pipe, mask_image=m, mask_dilate=[1, 2])
    for kw in (dict(mask_blur=2.0), dict(mask_dilate=1)):
        with pytest.raises(ValueError, match="mask_latents cannot be dilated or blurred"):
            _call(pipe, mask_image=None, mask_latents=torch.zeros(1, 1, 16, 16), **kw)


def test_all_zero_filtered_mask_with_crop_raises_on_the_host_route():
    from types import SimpleNamespace
    from PIL import Image
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import _InpaintImages
    image = Image.fromarray(np.zeros((64, 80, 3), np.uint8))
    zero = mask_filter_host(np.zeros((64, 80), np.uint8), 3, 4.0)
    with pytest.raises(ValueError, match="all zero"):
        _InpaintImages(SimpleNamespace(_device_image_io=False), image, zero, (128, 128), 8, "cpu")


# ---- the C ABI ----
@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def launchable_block():
    """fake, never dereferenced addresses: every refusal precedes the launch"""
    from imagdressing_amd import _lib
    p = _lib.ImageMaskFilterParams()
    p.src, p.out, p.tmp, p.bounds = 0x10000, 0x20000, 0x30000, 0x40000
    p.B, p.H, p.W = 2, 37, 53
    p.src_row_stride = p.out_row_stride = 53
    p.src_img_stride = p.out_img_stride = 37 * 53
    p.k, p.blur, p.passes = 3, 1, 3
    p.r, p.ww, p.fw = gaussian_box(4)
    return p


def refusals():
    """(field overrides, word of the error)"""
    r, ww, fw = gaussian_box(4)
    return [(dict(src=None), b"null pointer"), (dict(out=None), b"null pointer"),
            (dict(B=0), b"empty image"), (dict(H=0), b"empty image"), (dict(W=-1), b"empty image"),
            (dict(passes=2), b"passes (2) must be 3"), (dict(passes=0), b"passes (0) must be 3"), (dict(passes=4), b"passes (4) must be 3"),
            (dict(k=-1), b"k (-1)"),
            (dict(ww=ww + 1), b"inconsistent"), (dict(fw=fw + 1), b"inconsistent"), (dict(r=r + 1), b"inconsistent"), (dict(ww=0, fw=0), b"inconsistent"),
            (dict(src_row_stride=52), b"row stride"), (dict(out_row_stride=10), b"row stride"),
            (dict(src_img_stride=100), b"image stride"), (dict(out_img_stride=37 * 53 - 1), b"image stride"),
            (dict(H=1 << 16, W=1 << 16, src_row_stride=1 << 16, out_row_stride=1 << 16, B=1), b"exceeds 2^31 bytes"),
            (dict(flags=1, tmp=None), b"needs the uint8 plane tmp"),
            (dict(H=20000, src_img_stride=20000 * 53, out_img_stride=20000 * 53, tmp=None), b"needs the uint8 plane tmp"),
            (dict(flags=1, tmp=0x20000), b"plane of its own")]


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("imd_image_mask_filter", "imd_image_mask_filter_form"):
        assert name in declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "imd_image_mask_filter" in text
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    res, args = _lib.SYMBOLS["imd_image_mask_filter"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.ImageMaskFilterParams), ctypes.c_void_p]
    assert callable(ops.image_mask_filter)
    assert "image_filter.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "imagdressing_hip.h")).read()
    assert f"#define IMD_IMG_MASK_LINE_MAX {ops.IMAGE_MASK_LINE_MAX}" in header
    assert f"#define IMD_IMG_MASK_FORCE_GLOBAL {ops.IMAGE_MASK_FORCE_GLOBAL}" in header


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.ImageMaskFilterParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_image_mask_filter_params")
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    for ptr in ("src", "out", "tmp", "bounds"):
        assert kinds[ptr] is ctypes.c_void_p
    for s in ("src_row_stride", "src_img_stride", "out_row_stride", "out_img_stride"):
        assert kinds[s] is ctypes.c_int64
    for u in ("r", "ww", "fw"):
        assert kinds[u] is ctypes.c_uint32


def test_foreign_struct_size_is_refused(lib):
    from imagdressing_amd import _lib
    p = launchable_block()
    size = ctypes.sizeof(_lib.ImageMaskFilterParams)
    assert p.struct_bytes == size
    for bad in (size - 8, size + 8, ctypes.sizeof(_lib.ImageOverlayParams), 0):
        p.struct_bytes = bad
        assert lib.imd_image_mask_filter(ctypes.byref(p), None) != 0
        err = lib.imd_last_error()
        assert err.startswith(b"image_mask_filter:") and b"parameter block is" in err
        assert lib.imd_image_mask_filter_form(ctypes.byref(p)) == 0
    assert lib.imd_image_mask_filter(None, None) != 0 and b"image_mask_filter: null params" in lib.imd_last_error()


@pytest.mark.parametrize("case", range(len(refusals())))
def test_refusals_precede_the_launch(lib, case):
    over, word = refusals()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_image_mask_filter_form(ctypes.byref(p)) == 0
    assert lib.imd_image_mask_filter(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"image_mask_filter:") and word in err and b"launch failed" not in err, err


def test_launch_counts(lib):
    """what a call costs, without launching: 3 launches for both steps, 2 for one, 1 for none, one more for the bounds; a line past
    IMD_IMG_MASK_LINE_MAX (or the flag) one per pass"""
    def form(**over):
        p = launchable_block()
        p.bounds = None
        for k, v in over.items():
            setattr(p, k, v)
        return lib.imd_image_mask_filter_form(ctypes.byref(p))
    assert form() == 3 and form(k=0) == 2 and form(blur=0) == 2 and form(k=0, blur=0) == 1
    assert form(bounds=0x40000) == 4 and form(k=0, blur=0, bounds=0x40000) == 2
    assert form(flags=1) == 8 and form(flags=1, k=0) == 6 and form(flags=1, blur=0) == 2 and form(flags=1, k=0, blur=0) == 1
    assert form(H=16384, src_img_stride=16384 * 53, out_img_stride=16384 * 53) == 3
    assert form(H=16385, src_img_stride=16385 * 53, out_img_stride=16385 * 53) == 8
    assert form(blur=0, passes=7) == 2                                   # passes is read only with the Gaussian


def test_the_wrapper_has_no_cpu_path():
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    with pytest.raises(ImdError):
        ops.image_mask_filter(torch.zeros(1, 4, 4, dtype=torch.uint8), 1, gaussian_box(2))
