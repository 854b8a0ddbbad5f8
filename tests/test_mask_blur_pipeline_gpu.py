"""``mask_dilate`` / ``mask_blur`` of the inpainting pipeline on the GPU (small synthetic engines): the call equals the same call given
the Pillow-filtered mask, byte for byte, on the host route and on the device route -- with ``padding_mask_crop`` + ``overlay``, the
built-in inpaint condition, a caller's ``control_image``, the plain route, an RGB mask, and R = 2 requests of differing size with
per-request values; the device route never reaches ``Image.filter``; the defaults change neither a byte nor a launch; the crop box
read back from the device is ``get_crop_region`` of the Pillow-filtered mask."""
import numpy as np
import pytest
import torch

from tests.inpaint_cases import noise_image, rect_mask
from tests.test_image_io_gpu import common_kwargs, on_and_off, sched

pytestmark = pytest.mark.gpu

HW = (111, 150)
RECT = (30, 80, 40, 110)
K, BLUR = 3, 4.0


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    from imagdressing_amd.vae import AutoencoderKL
    from tests.harness import SMALL, build_pair
    from tests.test_vae_gpu import SMALL as VSMALL
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=torch.float16)
    vae = AutoencoderKL.random_init(seed=5, config=VSMALL, device="cuda", dtype=torch.float16)
    return IMAGDressing_v1(vae=vae, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=sched())


def pil(a):
    from PIL import Image
    return Image.fromarray(a)


def prefiltered(m, k, b):
    """the definition: m.convert("L").filter(MaxFilter(2k + 1)).filter(GaussianBlur(b)), a step whose value is 0 skipped"""
    from PIL import ImageFilter
    m = m.convert("L")
    if k:
        m = m.filter(ImageFilter.MaxFilter(2 * k + 1))
    if b:
        m = m.filter(ImageFilter.GaussianBlur(b))
    return m


def gray_mask():
    return pil(rect_mask(HW, RECT))


def rgb_mask():
    """an RGB mask whose "L" conversion is none of its channels"""
    m = rect_mask(HW, RECT)
    return pil(np.stack([m, m // 2, np.zeros_like(m)], -1))


def run(pipe, **kw):
    base = common_kwargs(1)
    base.update(image=pil(noise_image(2, HW)), control_image=pil(noise_image(3, HW)), output_type="np", generator=torch.Generator().manual_seed(7))
    base.update(kw)
    return pipe(**base).images


SCENARIOS = {
    "crop_overlay_condition": dict(padding_mask_crop=8, overlay=True, control_image=None),
    "crop_overlay_control": dict(padding_mask_crop=8, overlay=True),
    "condition_whole": dict(control_image=None),
    "plain_control": dict(),
    "overlay_whole_control": dict(overlay=True),
}


@pytest.mark.parametrize("mask", ["gray", "rgb"])
@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
@torch.no_grad()
def test_equals_the_call_with_the_prefiltered_mask(pipe, scenario, mask):
    from imagdressing_amd import ops
    kw = SCENARIOS[scenario]
    m = gray_mask() if mask == "gray" else rgb_mask()
    want_mask = prefiltered(m, K, BLUR)
    (a, b, c), deltas = on_and_off(pipe, lambda: run(pipe, mask_image=m, mask_dilate=K, mask_blur=BLUR, **kw))
    (wa, wb, wc), _ = on_and_off(pipe, lambda: run(pipe, mask_image=want_mask, **kw))
    for got, want in ((a, wa), (b, wb), (c, wc)):
        assert got.dtype == np.uint8 and torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))                       # and the two routes agree
    assert deltas[1]["mask_filter"] == 1 and deltas[0]["mask_filter"] == 0 and deltas[2]["mask_filter"] == 0
    assert deltas[1]["mask_filter_launches"] == (4 if "padding_mask_crop" in kw else 3)
    if kw.get("overlay"):
        plain = run(pipe, mask_image=m.convert("L"), **kw)
        assert not np.array_equal(plain, a)                                            # the filter is seen in the result


@torch.no_grad()
def test_one_step_alone(pipe):
    m = gray_mask()
    for k, b in ((K, 0.0), (0, 33.0)):
        (a, d, _), deltas = on_and_off(pipe, lambda: run(pipe, mask_image=m, mask_dilate=k, mask_blur=b, padding_mask_crop=8, overlay=True,
                                                         control_image=None))
        want = run(pipe, mask_image=prefiltered(m, k, b), padding_mask_crop=8, overlay=True, control_image=None)
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(want)) and torch.equal(torch.from_numpy(d), torch.from_numpy(want))
        assert deltas[1]["mask_filter_launches"] == 3                                  # two for the step, one for the bounds


@torch.no_grad()
def test_two_requests_of_differing_size_and_values(pipe):
    sizes = [(111, 150), (131, 97)]
    origs = [pil(noise_image(40 + r, sizes[r])) for r in range(2)]
    masks = [pil(rect_mask(sizes[0], RECT)), pil(np.stack([rect_mask(sizes[1], (40, 90, 20, 60))] * 3, -1))]
    ks, bs = [3, 0], [2.0, 7.25]
    want_masks = [prefiltered(masks[r], ks[r], bs[r]) for r in range(2)]
    kw = common_kwargs(2)
    kw.update(image=origs, control_image=None, padding_mask_crop=8, overlay=True, output_type="pil")

    def call(**over):
        return pipe(**dict(kw, generator=torch.Generator().manual_seed(7), **over)).images
    (a, b, c), deltas = on_and_off(pipe, lambda: call(mask_image=masks, mask_dilate=ks, mask_blur=bs))
    (wa, wb, wc), _ = on_and_off(pipe, lambda: call(mask_image=want_masks))
    for r in range(2):
        assert a[r].size == (sizes[r][1], sizes[r][0])
        assert a[r].tobytes() == wa[r].tobytes() and b[r].tobytes() == wb[r].tobytes() and c[r].tobytes() == wc[r].tobytes()
        assert a[r].tobytes() == b[r].tobytes()
    assert deltas[1]["mask_filter"] == 2 and deltas[0]["mask_filter"] == 0
    # one shared mask, filtered differently per request
    shared = dict(kw, image=origs[0])
    got = pipe(**dict(shared, generator=torch.Generator().manual_seed(7), mask_image=masks[0], mask_dilate=[1, 5], mask_blur=2.0)).images
    want = pipe(**dict(shared, generator=torch.Generator().manual_seed(7),
                       mask_image=[prefiltered(masks[0], 1, 2.0), prefiltered(masks[0], 5, 2.0)])).images
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    with pytest.raises(ValueError, match="entries for 2 requests"):
        call(mask_image=masks, mask_dilate=[1, 2, 3])


@torch.no_grad()
def test_plain_route_shared_mask_with_per_request_values(pipe):
    """R = 2 on the plain route (a caller's control_image, no crop, no overlay): one shared mask, grown by 1 and by 9 pixels"""
    kw = common_kwargs(2)
    kw.update(image=pil(noise_image(2, HW)), control_image=pil(noise_image(3, HW)), output_type="np")

    def call(**over):
        return pipe(**dict(kw, generator=torch.Generator().manual_seed(7), **over)).images
    (a, b, c), deltas = on_and_off(pipe, lambda: call(mask_image=gray_mask(), mask_dilate=[1, 9], mask_blur=[0.0, 3.0]))
    (wa, wb, wc), _ = on_and_off(pipe, lambda: call(mask_image=[prefiltered(gray_mask(), 1, 0.0), prefiltered(gray_mask(), 9, 3.0)]))
    for got, want in ((a, wa), (b, wb), (c, wc)):
        assert got.shape == (2, 128, 128, 3) and torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))
    assert deltas[1]["mask_filter"] == 2 and deltas[1]["mask_filter_launches"] == 2 + 3 and deltas[0]["mask_filter"] == 0
    same = call(mask_image=gray_mask(), mask_dilate=1)
    assert not np.array_equal(same[1], a[1])                                           # the second request's own values are seen


@torch.no_grad()
def test_device_route_never_reaches_pillow_filter(pipe, monkeypatch):
    from PIL import Image
    want = run(pipe, mask_image=prefiltered(gray_mask(), K, BLUR), padding_mask_crop=8, overlay=True, control_image=None)
    plain_want = run(pipe, mask_image=prefiltered(rgb_mask(), K, BLUR))

    def refuse(self, *a, **kw):
        raise AssertionError("Image.filter reached on the device route")
    monkeypatch.setattr(Image.Image, "filter", refuse)
    pipe.enable_device_image_io()
    try:
        got = run(pipe, mask_image=gray_mask(), mask_dilate=K, mask_blur=BLUR, padding_mask_crop=8, overlay=True, control_image=None)
        plain = run(pipe, mask_image=rgb_mask(), mask_dilate=K, mask_blur=BLUR)
    finally:
        pipe.disable_device_image_io()
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)) and torch.equal(torch.from_numpy(plain), torch.from_numpy(plain_want))
    with pytest.raises(AssertionError, match="Image.filter reached"):                  # (the host route does go through it)
        run(pipe, mask_image=gray_mask(), mask_dilate=K, mask_blur=BLUR)


class Recorder:
    """the loaded library, noting the name of every entry point called"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def noted(*a):
            self.calls.append(name)
            return fn(*a)
        return noted


@pytest.mark.parametrize("device_io", [False, True], ids=["host", "device"])
@torch.no_grad()
def test_defaults_change_nothing(pipe, device_io, monkeypatch):
    """mask_dilate=0, mask_blur=0.0 (scalars and per-request lists): the bytes and the list of library calls of a call without them"""
    from imagdressing_amd import _lib
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    pipe.enable_device_image_io(device_io)
    try:
        outs, lists = [], []
        for extra in (dict(), dict(mask_dilate=0, mask_blur=0.0), dict(mask_dilate=[0], mask_blur=[0.0])):
            rec.calls = []
            outs.append(run(pipe, mask_image=gray_mask(), padding_mask_crop=8, overlay=True, control_image=None, **extra))
            lists.append(list(rec.calls))
    finally:
        pipe.disable_device_image_io()
    assert len(lists[0]) > 10 and "imd_image_mask_filter" not in lists[0]
    assert lists[1] == lists[0] and lists[2] == lists[0]
    assert torch.equal(torch.from_numpy(outs[1]), torch.from_numpy(outs[0])) and torch.equal(torch.from_numpy(outs[2]), torch.from_numpy(outs[0]))


def test_crop_box_from_the_device_is_get_crop_region(pipe):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import _InpaintImages
    from imagdressing_amd.image import get_crop_region
    image = pil(noise_image(2, HW))
    seen_zero = False
    pipe.enable_device_image_io()
    try:
        for m in (gray_mask(), rgb_mask(), pil(rect_mask(HW, (5, 60, 100, 150))), pil(rect_mask(HW, (50, 51, 70, 71)))):
            for k, b in ((K, BLUR), (0, 33.0), (8, 0.0), (1, 0.3)):
                want = prefiltered(m, k, b)
                if not np.asarray(want).any():                     # (one pixel under radius 33 blurs to nothing: both refuse)
                    seen_zero = True
                    with pytest.raises(ValueError, match="all zero"):
                        get_crop_region(want, 128, 128, pad=8)
                    with pytest.raises(ValueError, match="all zero"):
                        _InpaintImages(pipe, image, m, (128, 128), 8, pipe.device, mask_filter=[(k, b)])
                    continue
                front = _InpaintImages(pipe, image, m, (128, 128), 8, pipe.device, mask_filter=[(k, b)])
                assert front.boxes == [get_crop_region(want, 128, 128, pad=8)], (k, b)
                assert torch.equal(front.uploaded("mask_l", 0)[0, ..., 0].cpu(), torch.from_numpy(np.array(want)))
    finally:
        pipe.disable_device_image_io()
    assert seen_zero


@torch.no_grad()
def test_errors_on_both_routes(pipe):
    zero = pil(np.zeros(HW, np.uint8))
    for flag in (False, True):
        pipe.enable_device_image_io(flag)
        try:
            with pytest.raises(ValueError, match="all zero"):
                run(pipe, mask_image=zero, mask_dilate=K, mask_blur=BLUR, padding_mask_crop=8)
            with pytest.raises(ValueError, match="mask_blur"):
                run(pipe, mask_image=gray_mask(), mask_blur=float("inf"))
            with pytest.raises(ValueError, match="mask_latents cannot be dilated or blurred"):
                run(pipe, mask_image=None, mask_latents=torch.zeros(1, 1, 16, 16, device="cuda"), mask_blur=2.0)
        finally:
            pipe.disable_device_image_io()


def test_mask_processor_of_the_pipeline(pipe):
    from PIL import ImageFilter
    m = gray_mask()
    assert pipe.mask_processor.blur(m, blur_factor=33).tobytes() == m.filter(ImageFilter.GaussianBlur(33)).tobytes()
    up = torch.from_numpy(np.array(m)).cuda()
    assert torch.equal(pipe.mask_processor.blur(up, blur_factor=33).cpu(), torch.from_numpy(np.array(m.filter(ImageFilter.GaussianBlur(33)))))
