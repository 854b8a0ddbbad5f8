"""Inpainting with padding_mask_crop / overlay without a GPU: the crop region against the pinned boxes and its invariants, the
single-rounding composite formula against Pillow's Image.composite on every byte triple, the host-route overlay and inpaint-condition
helpers, the C ABI of imd_image_overlay / imd_image_inpaint_condition, and the argument checks of the pipeline."""
import ctypes
import os
import types

import numpy as np
import pytest

from tests.inpaint_cases import (BOX_CASES, all_triples, case, case_mask, composite_formula, make_inpaint_condition, noise_image,
                                 rect_mask, soft_mask)
from tests.test_abi import declared_functions, header_struct_fields


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- crop region ----
@pytest.mark.parametrize("name", [c[0] for c in BOX_CASES])
def test_pinned_boxes(name):
    from PIL import Image
    from imagdressing_amd.image import get_crop_region
    _, hw, rect, extra, pad, (pw, ph), box = case(name)
    m = rect_mask(hw, rect, extra)
    assert get_crop_region(m, pw, ph, pad=pad) == box
    assert get_crop_region(Image.fromarray(m), pw, ph, pad=pad) == box                      # a PIL "L" mask
    assert get_crop_region(Image.fromarray(np.stack([m] * 3, -1)), pw, ph, pad=pad) == box  # ... and an RGB one, read as "L"
    assert get_crop_region(m[..., None], pw, ph, pad=pad) == box


def test_all_zero_mask_raises():
    from imagdressing_amd.image import get_crop_region
    with pytest.raises(ValueError, match="all zero"):
        get_crop_region(np.zeros((111, 150), np.uint8), 128, 128, pad=8)


def test_boxes_lie_inside_the_image_and_keep_the_processing_aspect():
    """400 seeded rectangles.  The box is inside the image; the axis that the region grows along reaches the processing aspect to
    within one pixel (the int() of step 3) whenever the image has room for it."""
    from imagdressing_amd.image import get_crop_region
    rng = np.random.default_rng(11)
    grown = 0
    for _ in range(400):
        h, w = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        t, l = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
        b, r = int(rng.integers(t + 1, h + 1)), int(rng.integers(l + 1, w + 1))
        pad = int(rng.integers(0, 20))
        pw, ph = [(128, 128), (96, 128), (512, 640), (640, 512)][int(rng.integers(0, 4))]
        x1, y1, x2, y2 = get_crop_region(rect_mask((h, w), (t, b, l, r)), pw, ph, pad=pad)
        assert 0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h
        px1, py1, px2, py2 = max(l - pad, 0), max(t - pad, 0), min(r + pad, w), min(b + pad, h)     # steps 1 and 2
        assert x1 <= px1 and y1 <= py1 and x2 >= px2 and y2 >= py2                                   # step 3 only grows
        rp = pw / ph
        if (px2 - px1) / (py2 - py1) > rp:
            assert (x1, x2) == (px1, px2)
            want = (x2 - x1) / rp
            if want <= h:
                assert abs((y2 - y1) - want) <= 1
                grown += 1
        else:
            assert (y1, y2) == (py1, py2)
            want = (y2 - y1) * rp
            if want <= w:
                assert abs((x2 - x1) - want) <= 1
                grown += 1
    assert grown > 100


# ---- the composite ----
def test_formula_equals_pillow_composite_on_every_triple():
    from PIL import Image
    orig, gen, m = all_triples()
    assert np.unique(orig[..., 0].astype(np.uint32) << 16 | gen[..., 0].astype(np.uint32) << 8 | m).size == 1 << 24
    want = np.asarray(Image.composite(Image.fromarray(gen), Image.fromarray(orig), Image.fromarray(m)))
    got = composite_formula(orig, gen, m[..., None])
    assert np.array_equal(got, want)
    assert np.array_equal(got[m == 0], orig[m == 0]) and np.array_equal(got[m == 255], gen[m == 255])


@pytest.mark.parametrize("name", ["A", "C", "G"])
def test_host_overlay_equals_the_pillow_calls(name):
    from PIL import Image
    from imagdressing_amd.image import overlay_host, overlay_reference, resample_reference
    _, hw, rect, _, _, _, box = case(name)
    x1, y1, x2, y2 = box
    orig, gen = noise_image(1, hw), noise_image(2, (128, 128))
    mask = soft_mask(hw, rect, 3)
    assert (mask[y1:y2, x1:x2] == 0).any() and (mask[y1:y2, x1:x2] == 255).any() and len(np.unique(mask[y1:y2, x1:x2])) > 20
    got = overlay_host(gen, Image.fromarray(orig), Image.fromarray(mask), box)
    assert got.mode == "RGB" and got.size == (hw[1], hw[0])
    gen_r = Image.fromarray(gen).resize((x2 - x1, y2 - y1), Image.LANCZOS)
    base = Image.fromarray(orig).copy()
    base.paste(gen_r, (x1, y1))
    want = np.asarray(Image.composite(base, Image.fromarray(orig), Image.fromarray(mask)))
    got = np.asarray(got)
    assert np.array_equal(got, want)
    # ... and the integer formulas (what the device route computes)
    assert np.array_equal(got, overlay_reference(orig, resample_reference(gen, (y2 - y1, x2 - x1), "lanczos"), mask, box))
    outside = np.ones(hw, bool)
    outside[y1:y2, x1:x2] = False
    assert np.array_equal(got[outside], orig[outside]) and np.array_equal(got[mask == 0], orig[mask == 0])
    assert not np.array_equal(got, orig)


@pytest.mark.parametrize("name", ["A", "G", None])
def test_host_inpaint_condition_equals_the_script_function(name):
    from PIL import Image
    from imagdressing_amd.image import inpaint_condition_host
    hw, rect, box = ((111, 150), (30, 80, 40, 110), None) if name is None else (case(name)[1], case(name)[2], case(name)[6])
    img, mask = Image.fromarray(noise_image(4, hw)), Image.fromarray(soft_mask(hw, rect, 5))
    got = inpaint_condition_host(img, mask, box, (128, 120))
    win_i, win_m = (img, mask) if box is None else (img.crop(box), mask.crop(box))
    want = make_inpaint_condition(win_i.resize((120, 128), Image.LANCZOS), win_m.convert("L").resize((120, 128), Image.LANCZOS))
    assert got.dtype == np.float32 and got.shape == (128, 120, 3) and np.array_equal(got, want)
    assert (got == -1).all(-1).any() and (got >= 0).all(-1).any()


# ---- C ABI ----
def test_entry_points_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    for name in ("imd_image_overlay", "imd_image_inpaint_condition"):
        assert name in declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive: the version stays
    assert {"overlay", "inpaint_condition", "resample", "pack_u8"} <= set(ops.IMAGE_IO_COUNTER)
    from imagdressing_amd import image
    assert "get_crop_region" in image.__all__


@pytest.mark.parametrize("cname,pyname", [("imd_image_overlay_params", "ImageOverlayParams"),
                                          ("imd_image_inpaint_condition_params", "ImageInpaintConditionParams")])
def test_struct_layout_matches_header(cname, pyname):
    from imagdressing_amd import _lib
    fields = getattr(_lib, pyname)._fields_
    assert [f[0] for f in fields] == header_struct_fields(cname)
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    for name, kind in fields[1:]:
        assert kind is (ctypes.c_void_p if name in ("orig", "mask", "gen", "out", "image") else ctypes.c_int), name


def overlay_block():
    """B = 2 over one shared 111 x 150 image, box A: a block that would launch (addresses are never dereferenced on the host)"""
    from imagdressing_amd import _lib
    p = _lib.ImageOverlayParams()
    p.orig, p.mask, p.gen, p.out = 0x10000, 0x30000, 0x40000, 0x80000
    p.B, p.Bo, p.H0, p.W0 = 2, 1, 111, 150
    p.x1, p.y1, p.cw, p.ch = 32, 12, 86, 86
    return p


def condition_block():
    from imagdressing_amd import _lib
    p = _lib.ImageInpaintConditionParams()
    p.image, p.mask, p.out = 0x10000, 0x30000, 0x40000
    p.B, p.H, p.W, p.dtype = 1, 128, 128, 1
    return p


def test_foreign_struct_size_and_null_params_are_refused(lib):
    for make, fn, word in ((overlay_block, lib.imd_image_overlay, b"image_overlay"),
                           (condition_block, lib.imd_image_inpaint_condition, b"image_inpaint_condition")):
        size = make().struct_bytes
        for bad in (size - 8, size + 8, 0):
            p = make()
            p.struct_bytes = bad
            assert fn(ctypes.byref(p), None) != 0
            assert word in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
        assert fn(None, None) != 0 and b"null params" in lib.imd_last_error()


@pytest.mark.parametrize("over,word", [
    (dict(orig=None), b"null pointer"), (dict(mask=None), b"null pointer"), (dict(gen=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(x1=65), b"outside the image"), (dict(y1=26), b"outside the image"), (dict(x1=-1), b"outside the image"),
    (dict(y1=-1), b"outside the image"), (dict(cw=151, x1=0), b"outside the image"), (dict(ch=112, y1=0), b"outside the image"),
    (dict(x1=2 ** 31 - 1), b"outside the image"), (dict(cw=0), b"empty box"), (dict(ch=0), b"empty box"), (dict(cw=-3), b"empty box"),
    (dict(Bo=3), b"Bo (3) must be 1"), (dict(B=0), b"empty image"), (dict(W0=0), b"empty image"),
    (dict(H0=30000, W0=30000), b"exceeds 2^31 bytes")])
def test_overlay_refusals_precede_the_launch(lib, over, word):
    p = overlay_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_image_overlay(ctypes.byref(p), None) != 0
    assert word in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error(), lib.imd_last_error()


@pytest.mark.parametrize("over,word", [(dict(image=None), b"null pointer"), (dict(mask=None), b"null pointer"), (dict(out=None), b"null pointer"),
                                       (dict(B=0), b"empty image"), (dict(dtype=5), b"unknown dtype 5"), (dict(out=0x40008), b"16-byte")])
def test_inpaint_condition_refusals_precede_the_launch(lib, over, word):
    p = condition_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_image_inpaint_condition(ctypes.byref(p), None) != 0
    assert word in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error(), lib.imd_last_error()


def test_new_image_ops_have_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)          # noqa: E731
    with pytest.raises(ImdError):
        ops.image_overlay(u8(1, 8, 8, 3), u8(1, 8, 8), u8(1, 4, 4, 3), (0, 0, 4, 4))
    with pytest.raises(ImdError):
        ops.image_inpaint_condition(u8(1, 8, 8, 3), u8(1, 8, 8), torch.float16)


# ---- the pipeline's argument checks (raised before any GPU work) ----
def cpu_pipe():
    import torch
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    engine = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float16, attn_processors={})
    return IMAGDressing_v1(vae=None, reference_unet=engine, unet=engine, tokenizer=None, text_encoder=None, controlnet=engine,
                           image_encoder=None, ImgProj=lambda h: h, scheduler=None)


def call_kwargs(**over):
    import torch
    from PIL import Image
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=3,
              guidance_scale=5.0, prompt_embeds=torch.zeros(1, 77, 64), negative_prompt_embeds=torch.zeros(1, 77, 64),
              ref_clip_hidden_states=torch.zeros(1, 16, 64), ref_image_latents=torch.zeros(1, 4, 16, 16),
              image=Image.fromarray(noise_image(1, (111, 150))), mask_image=Image.fromarray(case_mask("A")),
              control_image=Image.fromarray(noise_image(2, (111, 150))))
    kw.update(over)
    return kw


def test_pipeline_value_errors():
    import torch
    from PIL import Image
    pipe = cpu_pipe()
    small = Image.fromarray(noise_image(3, (100, 150)))
    with pytest.raises(ValueError, match="equal size"):
        pipe(**call_kwargs(padding_mask_crop=8, image=small))
    with pytest.raises(ValueError, match="cannot be cropped"):
        pipe(**call_kwargs(padding_mask_crop=8, image_latents=torch.zeros(1, 4, 16, 16)))
    with pytest.raises(ValueError, match="cannot be cropped"):
        pipe(**call_kwargs(padding_mask_crop=8, mask_latents=torch.zeros(1, 1, 16, 16)))
    with pytest.raises(ValueError, match="all zero"):
        pipe(**call_kwargs(padding_mask_crop=8, mask_image=Image.fromarray(np.zeros((111, 150), np.uint8))))
    with pytest.raises(ValueError, match="PIL image or uint8 array"):
        pipe(**call_kwargs(padding_mask_crop=8, image=torch.zeros(1, 3, 111, 150)))
    with pytest.raises(ValueError, match=r"float \[\*, 3, 111, 150\] tensor of the image's size"):
        pipe(**call_kwargs(padding_mask_crop=8, control_image=torch.zeros(1, 3, 128, 128)))
    with pytest.raises(ValueError, match="control_image is"):
        pipe(**call_kwargs(padding_mask_crop=8, control_image=small))
    # overlay
    for bad in ("pt", "latent"):
        with pytest.raises(ValueError, match="'pil' or 'np'"):
            pipe(**call_kwargs(overlay=True, output_type=bad))
    with pytest.raises(ValueError, match="PIL image or uint8 array"):
        pipe(**call_kwargs(overlay=True, image=None, image_latents=torch.zeros(1, 4, 16, 16)))
    with pytest.raises(ValueError, match="PIL image or uint8 array"):
        pipe(**call_kwargs(overlay=True, mask_image=torch.zeros(1, 1, 111, 150)))
    two = dict(prompt_embeds=torch.zeros(2, 77, 64), image=[Image.fromarray(noise_image(1, (111, 150))), Image.fromarray(noise_image(2, (131, 97)))],
               mask_image=[Image.fromarray(case_mask("A")), Image.fromarray(case_mask("G"))])
    with pytest.raises(ValueError, match="'pil'"):
        pipe(**call_kwargs(overlay=True, output_type="np", **two))
    # what stays refused
    with pytest.raises(NotImplementedError):
        pipe(**call_kwargs(padding_mask_crop=8, guess_mode=True))
    with pytest.raises(NotImplementedError):
        pipe(**call_kwargs(timesteps=[1, 2]))
    with pytest.raises(NotImplementedError):
        pipe(**call_kwargs(guidance_scale=1.0))


def test_overlay_is_appended_to_the_call_signature():
    import inspect
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    sig = inspect.signature(IMAGDressing_v1.__call__)
    names = list(sig.parameters)
    assert names[-2:] == ["overlay", "kwargs"] and sig.parameters["overlay"].default is False
    assert sig.parameters["padding_mask_crop"].default is None
