"""Inpainting crop / overlay on the GPU: imd_image_overlay against the numpy formula on every (orig, gen, mask) byte triple and on
box geometries whose rows and box edges are not 16-byte aligned (with a guard band behind the output), imd_image_inpaint_condition
against the host expression, and the inpainting pipeline with ``padding_mask_crop``, ``control_image=None`` and ``overlay=True``:
the device image route against the default route, byte for byte."""
import numpy as np
import pytest
import torch

from tests.inpaint_cases import all_triples, case, case_mask, composite_formula, make_inpaint_condition, noise_image, soft_mask
from tests.test_image_io_gpu import common_kwargs, on_and_off, sched

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.vae import AutoencoderKL
    from tests.harness import SMALL, build_pair
    from tests.test_vae_gpu import SMALL as VSMALL
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=torch.float16)
    p["vae"] = AutoencoderKL.random_init(seed=5, config=VSMALL, device="cuda", dtype=torch.float16)
    return p


@pytest.fixture(scope="module")
def pipe(engines):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    p = engines
    return IMAGDressing_v1(vae=p["vae"], reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=sched())


# ---- kernels ----
def test_overlay_every_triple(engines):
    """one launch over [1, 4096, 4096, 3]: all 256^3 (orig, gen, mask) triples in channel 0, two more bijections in channels 1 and 2;
    the box is the whole image, so every lane takes the 16-byte path"""
    from imagdressing_amd import ops
    orig, gen, m = all_triples()
    want = torch.from_numpy(composite_formula(orig, gen, m[..., None]))
    got = ops.image_overlay(torch.from_numpy(orig)[None].cuda(), torch.from_numpy(m)[None].cuda(), torch.from_numpy(gen)[None].cuda(),
                            (0, 0, 4096, 4096))
    assert got.shape == (1, 4096, 4096, 3) and got.dtype == torch.uint8
    assert torch.equal(got[0].cpu(), want)


@pytest.mark.parametrize("shared", [True, False], ids=["B3_shared", "B2_own"])
@pytest.mark.parametrize("name", ["A", "C", "E", "G"])
def test_overlay_geometry(engines, name, shared):
    """111 x 150: rows of 450 bytes, not a multiple of 16, so lanes straddle rows, box edges and (49950 bytes an image) images;
    131 x 97 with the 7 x 7 box G; rows of gen start at arbitrary byte offsets.  The output sits at a 5-byte offset inside a buffer
    filled with a guard value: nothing before or behind it may change."""
    from imagdressing_amd import ops
    from imagdressing_amd.image import overlay_reference
    _, hw, rect, _, _, _, box = case(name)
    x1, y1, x2, y2 = box
    B, Bo = (3, 1) if shared else (2, 2)
    orig = np.stack([noise_image(10 + i, hw) for i in range(Bo)])
    mask = np.stack([soft_mask(hw, rect, 20 + i) for i in range(Bo)])
    gen = np.stack([noise_image(30 + i, (y2 - y1, x2 - x1)) for i in range(B)])
    n = B * hw[0] * hw[1] * 3
    buf = torch.full((5 + n + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    out = buf[5:5 + n].view(B, hw[0], hw[1], 3)
    got = ops.image_overlay(torch.from_numpy(orig).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(gen).cuda(), box, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = overlay_reference(orig, gen, mask, box)
    assert want.shape == (B,) + hw + (3,)
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    outside = np.ones(hw, bool)
    outside[y1:y2, x1:x2] = False
    assert np.array_equal(got[:, outside], np.broadcast_to(orig, got.shape)[:, outside])
    assert (buf[:5] == GUARD).all() and (buf[5 + n:] == GUARD).all()
    if name != "E":
        assert not np.array_equal(got, np.broadcast_to(orig, got.shape))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_inpaint_condition_kernel(engines, dtype):
    """every mask value 0..255 (127 / 255 < 0.5 < 128 / 255) against every image value, B = 2"""
    from imagdressing_amd import ops
    v = np.arange(256, dtype=np.uint8)
    mask = np.stack([np.broadcast_to(v[:, None], (256, 256)), np.broadcast_to(v[None, :], (256, 256))]).copy()
    image = np.stack([np.stack([np.broadcast_to(v[None, :], (256, 256)), noise_image(1, (256, 256), 0), noise_image(2, (256, 256), 0)], -1),
                      noise_image(3, (256, 256))])
    got = ops.image_inpaint_condition(torch.from_numpy(image).cuda(), torch.from_numpy(mask).cuda(), dtype)
    assert got.shape == (2, 256, 256, 8) and got.dtype == dtype
    want = np.stack([make_inpaint_condition(image[b], mask[b]) for b in range(2)])
    assert want.dtype == np.float32 and (want[0, 128:] == -1).all() and (want[0, :128] >= 0).all()
    assert torch.equal(got[..., :3].cpu(), torch.from_numpy(want).to(dtype)) and not got[..., 3:].any()
    got4 = ops.image_inpaint_condition(torch.from_numpy(image).cuda(), torch.from_numpy(mask[..., None].copy()).cuda(), dtype)   # [B, H, W, 1]
    assert torch.equal(got4, got)


# ---- the pipeline ----
def pil(a):
    from PIL import Image
    return Image.fromarray(a)


def banded_mask():
    """mask A (255 on rows 30:80, cols 40:110 of 111 x 150) with grey noise 1..20 in a band around it -- rows 20:95, cols 25:125 --
    and zero beyond: the crop region follows the non-zero band, not the rectangle (box A would be (32, 12, 118, 98)), and is not the
    whole image either, so the cropped call differs from the uncropped one.  Every noise level binarises to 0."""
    m = np.zeros((111, 150), np.uint8)
    m[20:95, 25:125] = np.random.default_rng(9).integers(1, 21, size=(75, 100), dtype=np.uint8)
    m[30:80, 40:110] = 255
    return m


BAND_BOX = (17, 0, 133, 111)


def test_banded_mask_box():
    from imagdressing_amd.image import get_crop_region
    assert get_crop_region(banded_mask(), 128, 128, pad=8) == BAND_BOX != case("A")[6]


def run(pipe, **kw):
    base = common_kwargs(1)
    base.update(image=pil(noise_image(2, (111, 150))), mask_image=pil(banded_mask()), control_image=pil(noise_image(3, (111, 150))),
                output_type="np", generator=torch.Generator().manual_seed(7))
    base.update(kw)
    return pipe(**base).images


@torch.no_grad()
def test_pipeline_crop_only(pipe):
    (a, b, c), deltas = on_and_off(pipe, lambda: run(pipe, padding_mask_crop=8))
    assert a.shape == (1, 128, 128, 3) and a.dtype == np.uint8 and a.std() > 1          # the repainted window at the processing size
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert deltas[1]["resample"] == 3 and deltas[1]["pack_u8"] == 1                       # person image, mask, control image windows
    assert deltas[1]["overlay"] == 0 and deltas[1]["inpaint_condition"] == 0
    assert not any(deltas[0].values()) and not any(deltas[2].values())
    plain = run(pipe)
    assert plain.shape == a.shape and not np.array_equal(plain, a)
    # uint8 arrays are taken like PIL images
    arr = run(pipe, padding_mask_crop=8, image=noise_image(2, (111, 150)), mask_image=banded_mask(), control_image=noise_image(3, (111, 150)))
    assert np.array_equal(arr, a)


@torch.no_grad()
def test_pipeline_float_tensor_control_image(pipe):
    cond = torch.from_numpy(make_inpaint_condition(noise_image(2, (111, 150)), banded_mask())).permute(2, 0, 1)[None]
    assert cond.shape == (1, 3, 111, 150) and (cond == -1).any()
    (a, b, c), deltas = on_and_off(pipe, lambda: run(pipe, padding_mask_crop=8, control_image=cond))
    assert a.shape == (1, 128, 128, 3) and np.array_equal(a, b) and np.array_equal(a, c)
    assert deltas[1]["resample"] == 2 and not any(deltas[0].values())
    assert not np.array_equal(a, run(pipe, padding_mask_crop=8))


@pytest.mark.parametrize("crop", [8, None], ids=["crop", "whole"])
@torch.no_grad()
def test_pipeline_builds_the_inpaint_condition(pipe, crop):
    (a, b, c), deltas = on_and_off(pipe, lambda: run(pipe, padding_mask_crop=crop, control_image=None))
    assert a.shape == (1, 128, 128, 3) and np.array_equal(a, b) and np.array_equal(a, c)
    assert deltas[1]["inpaint_condition"] == 1 and deltas[1]["pack_u8"] == 1
    assert not any(deltas[0].values()) and not any(deltas[2].values())
    assert not np.array_equal(a, run(pipe, padding_mask_crop=crop))


def overlay_mask():
    """soft inside the band box: every grey level around rectangle A, zero beyond -- the seam is feathered and m == 0 occurs in the box"""
    return soft_mask((111, 150), (30, 80, 40, 110), 6)


@pytest.mark.parametrize("output_type", ["np", "pil"])
@pytest.mark.parametrize("crop", [8, None], ids=["crop", "whole"])
@torch.no_grad()
def test_pipeline_overlay(pipe, crop, output_type):
    from imagdressing_amd.image import get_crop_region
    orig, m = noise_image(2, (111, 150)), overlay_mask()
    box = get_crop_region(m, 128, 128, pad=8) if crop else (0, 0, 150, 111)
    x1, y1, x2, y2 = box
    assert crop is None or (0 < x1 and x2 < 150)
    (a, b, c), deltas = on_and_off(pipe, lambda: run(pipe, padding_mask_crop=crop, overlay=True, mask_image=pil(m), output_type=output_type))
    if output_type == "pil":
        assert all(len(o) == 1 and o[0].mode == "RGB" and o[0].size == (150, 111) for o in (a, b, c))
        a, b, c = (np.asarray(o[0])[None] for o in (a, b, c))
    assert a.shape == (1, 111, 150, 3) and a.dtype == np.uint8                            # the original's size
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert deltas[1]["overlay"] == 1 and deltas[1]["pack_u8"] == 1 and deltas[1]["resample"] == 4      # three inputs, the decoded window
    assert not any(deltas[0].values()) and not any(deltas[2].values())
    assert (m[y1:y2, x1:x2] == 0).any() and np.array_equal(a[0][m == 0], orig[m == 0])
    outside = np.ones((111, 150), bool)
    outside[y1:y2, x1:x2] = False
    assert np.array_equal(a[0][outside], orig[outside])
    assert not np.array_equal(a[0][m == 255], orig[m == 255])


@torch.no_grad()
def test_pipeline_two_requests_of_differing_size(pipe):
    """R = 2: images of 111 x 150 and 131 x 97, own masks and boxes, "pil".  The rows of a batched call are NOT bit-identical to solo
    calls here (tile configs depend on the row count: tests/test_multi_request_gpu.py::test_batched_matches_solo_calls), so the
    per-request comparison is made on the overlay stage alone: the decoded batch of the same R = 2 call (overlay off) goes through the
    host helper and through DeviceImageProcessor.overlay per request, and both must give the pipeline's overlay=True rows."""
    from imagdressing_amd.image import DeviceImageProcessor, get_crop_region, overlay_host
    sizes = [(111, 150), (131, 97)]
    origs = [noise_image(40 + r, sizes[r]) for r in range(2)]
    masks = [soft_mask(sizes[0], (30, 80, 40, 110), 6), soft_mask(sizes[1], (40, 90, 20, 60), 7)]
    boxes = [get_crop_region(masks[r], 128, 128, pad=8) for r in range(2)]
    assert boxes[0] != boxes[1]
    kw = common_kwargs(2)
    kw.update(image=[pil(o) for o in origs], mask_image=[pil(m) for m in masks], control_image=None, padding_mask_crop=8,
              generator=torch.Generator().manual_seed(7))

    def call(**over):
        kw["generator"] = torch.Generator().manual_seed(7)
        return pipe(**dict(kw, **over)).images
    (a, b, c), deltas = on_and_off(pipe, lambda: call(overlay=True, output_type="pil"))
    assert deltas[1]["overlay"] == 2 and deltas[1]["inpaint_condition"] == 2 and deltas[1]["pack_u8"] == 1
    assert not any(deltas[0].values())
    for r in range(2):
        assert a[r].size == (sizes[r][1], sizes[r][0])
        assert a[r].tobytes() == b[r].tobytes() == c[r].tobytes()
    decoded = call(output_type="np")                                                       # [2, 128, 128, 3], default route
    assert decoded.shape == (2, 128, 128, 3)
    proc = DeviceImageProcessor("cuda", torch.float16)
    for r in range(2):
        x1, y1, x2, y2 = boxes[r]
        host = np.asarray(overlay_host(decoded[r], pil(origs[r]), pil(masks[r]), boxes[r]))
        dev = proc.overlay(torch.from_numpy(decoded[r:r + 1]).cuda(), pil(origs[r]), pil(masks[r]), boxes[r])[0].cpu().numpy()
        assert np.array_equal(host, dev) and np.array_equal(host, np.asarray(a[r]))
        outside = np.ones(sizes[r], bool)
        outside[y1:y2, x1:x2] = False
        assert np.array_equal(host[outside], origs[r][outside]) and np.array_equal(host[masks[r] == 0], origs[r][masks[r] == 0])
    with pytest.raises(ValueError, match="'pil'"):
        call(overlay=True, output_type="np")
