"""Image I/O on the GPU: imd_image_resample against the recorded Pillow results (tests/golden/image_io.npz) bit for bit -- one launch
and the two-launch fallback, C = 3 and 1, crop windows, the three output kinds, binarise -- CLIPImageProcessor's recorded pixel values,
imd_image_pack_u8 against the host formula of ``_decode`` on every 16-bit value, and the pipelines with ``enable_device_image_io()``
against their default path, bit for bit."""
import numpy as np
import pytest
import torch

from tests.image_golden import CASES, FILTERS, clip_case, golden_case, load

pytestmark = pytest.mark.gpu

CROP = (5, 3, 29, 37)          # (top, left, h, w): does not start at 0, odd width, inside every case's output


@pytest.fixture(scope="module")
def golden():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return load()


def pair_of(x):
    """B = 2: the golden input and its point reflection"""
    return np.stack([x, x[::-1, ::-1].copy()])


def resize(x, size, filt, **kw):
    from imagdressing_amd.image import resize_to
    return resize_to(torch.from_numpy(np.ascontiguousarray(x)).cuda(), size, filt, **kw)


def forms_run(fn):
    """fn() -> (its result, the two-axis launch forms it took: {'resample_single': n, 'resample_two_pass': m} deltas)"""
    from imagdressing_amd import ops
    before = dict(ops.IMAGE_IO_COUNTER)
    out = fn()
    return out, {k: ops.IMAGE_IO_COUNTER[k] - before[k] for k in ("resample_single", "resample_two_pass")}


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_resample_u8_equals_recorded_pillow(golden, case, filt):
    from imagdressing_amd.image import resample_reference
    x, want = golden_case(golden, case, filt)
    hin, win, hout, wout = CASES[case]
    both_axes = hin != hout and win != wout
    xs = pair_of(x)
    ref1 = resample_reference(xs[1], (hout, wout), filt)           # (the integer formula: equal to Pillow on every golden case, on the CPU)
    for C in (3, 1):
        for force in (False, True):
            got, forms = forms_run(lambda: resize(xs[..., :C], (hout, wout), filt, _force_two_pass=force))
            assert got.shape == (2, hout, wout, C) and got.dtype == torch.uint8
            got = got.cpu().numpy()
            assert np.array_equal(got[0], want[..., :C]), (C, force, int(np.abs(got[0].astype(int) - want[..., :C]).max()))
            assert np.array_equal(got[1], ref1[..., :C]), (C, force)
            # which form ran: the strong reduction (203, 155) -> (24, 24) included, every golden case fits the LDS tile by itself
            assert forms == (dict(resample_single=int(not force), resample_two_pass=int(force)) if both_axes
                             else dict(resample_single=0, resample_two_pass=0)), (forms, C, force)


@pytest.mark.parametrize("C", [3, 1])
def test_tall_reduction_selects_the_two_launch_form_by_itself(golden, C):
    """1200 rows -> 8 with Lanczos: one tile reads all 1200 rows of the horizontal pass, more than its LDS holds (341 rows at C = 3,
    1024 at C = 1)"""
    from imagdressing_amd import ops
    from imagdressing_amd.image import resample_reference
    assert 1200 * ops.IMAGE_TILE_W * C > ops.IMAGE_LDS_BYTES
    x = np.random.default_rng(3).integers(0, 256, size=(2, 1200, 12, C), dtype=np.uint8)
    got, forms = forms_run(lambda: resize(x, (8, 8), "lanczos"))
    assert forms == dict(resample_single=0, resample_two_pass=1)
    assert np.array_equal(got.cpu().numpy(), resample_reference(x, (8, 8), "lanczos"))
    got, forms = forms_run(lambda: resize(x, (8, 8), "lanczos", crop=(1, 2, 6, 5)))
    assert forms == dict(resample_single=0, resample_two_pass=1)
    assert np.array_equal(got.cpu().numpy(), resample_reference(x, (8, 8), "lanczos")[:, 1:7, 2:7])


@pytest.mark.parametrize("case", [0, 2, 3, 4, 5])
def test_crop_window(golden, case):
    filt = "lanczos" if case != 2 else "bicubic"
    x, want = golden_case(golden, case, filt)
    hout, wout = CASES[case][2:]
    crop = CROP if case != 2 else (5, 3, 17, 19)                    # (the 24 x 24 output)
    t, l, h, w = crop
    for C in (3, 1):
        for force in (False, True):
            got = resize(pair_of(x)[..., :C], (hout, wout), filt, crop=crop, _force_two_pass=force)
            assert got.shape == (2, h, w, C)
            assert np.array_equal(got[0].cpu().numpy(), want[t:t + h, l:l + w, :C]), (C, force)


@pytest.mark.parametrize("size", [(64, 80), (70, 85), (111, 150), (24, 24)])
@pytest.mark.parametrize("normalize", [True, False])
def test_f32_nchw_equals_to_image_tensor(golden, size, normalize):
    """a = 2, b = -1 (normalize) and a = 1, b = 0: the values of the pipelines' host route on a PIL input, bit for bit"""
    from PIL import Image
    from imagdressing_amd.dressing_sd.pipelines._base import to_image_tensor
    from imagdressing_amd.image import DeviceImageProcessor
    pil = [Image.fromarray(golden["in_97x131"]), Image.fromarray(golden["in_203x155"])]
    want = to_image_tensor(pil, "cpu", normalize=normalize, size=size)
    got = DeviceImageProcessor("cuda", torch.float16).preprocess(pil, size=size, out="nchw", normalize=normalize)
    assert got.dtype == torch.float32 and got.shape == want.shape == (2, 3, size[0] // 8 * 8, size[1] // 8 * 8)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_nhwc8_equals_nchw_to_nhwc8(golden, dtype, mode):
    from imagdressing_amd.image import DeviceImageProcessor
    from imagdressing_amd.unet import nchw_to_nhwc8
    C = 3 if mode == "RGB" else 1
    imgs = [golden["in_97x131"][..., :C], golden["in_50x37"][..., :C]]
    proc = DeviceImageProcessor("cuda", dtype)
    for normalize in (True, False):
        nchw = proc.preprocess(imgs, size=(64, 80), out="nchw", normalize=normalize, mode=mode)
        got = proc.preprocess(imgs, size=(64, 80), out="nhwc8", normalize=normalize, mode=mode)
        assert got.shape == (2, 64, 80, 8) and got.dtype == dtype
        assert torch.equal(got, nchw_to_nhwc8(nchw, dtype))
        assert (got[..., C:] == 0).all() and got[..., :C].float().abs().max() > 0.5


def test_arbitrary_affine_map_is_not_contracted(golden):
    """y = (float(v) / 255) * a + b with one rounding per operation: equal to numpy's fp32 evaluation bit for bit"""
    from imagdressing_amd import ops
    x, want = golden_case(golden, 0, "bicubic")
    a = np.asarray([3.7226166, 0.3333333, -1.9], np.float32)
    b = np.asarray([-1.7922626, 0.1234567, 0.7], np.float32)
    got = resize(x[None], (64, 80), "bicubic", kind=ops.IMAGE_F32_NCHW, a=a, b=b)
    ref = ((want.astype(np.float32) / np.float32(255.0)) * a + b).transpose(2, 0, 1)
    assert ref.dtype == np.float32 and np.array_equal(got[0].cpu().numpy(), ref)


@pytest.mark.parametrize("case", [0, 5])
def test_binarize_equals_thresholding_the_golden(golden, case):
    from imagdressing_amd import ops
    x, want = golden_case(golden, case, "lanczos")
    hout, wout = CASES[case][2:]
    bits = (want.astype(np.float32) / np.float32(255.0)) >= 0.5
    assert 0.2 < bits.mean() < 0.8
    for C in (3, 1):
        u8 = resize(x[None, ..., :C], (hout, wout), "lanczos", binarize=True)
        assert np.array_equal(u8[0].cpu().numpy(), np.where(bits[..., :C], 255, 0).astype(np.uint8))
        f32 = resize(x[None, ..., :C], (hout, wout), "lanczos", binarize=True, kind=ops.IMAGE_F32_NCHW)
        assert np.array_equal(f32[0].cpu().numpy(), bits[..., :C].transpose(2, 0, 1).astype(np.float32))


def test_clip_preprocess_equals_recorded_transformers(golden):
    """Compares the ROWS the golden records (every 8th and the last of the 224, all columns and channels: the file stays under 300 KB;
    the resize underneath is compared exactly, on every pixel, by the resample tests).  |diff| <= 1e-5 in fp32: values reach ~2.6 (fp32 spacing 2.4e-7); three roundings here and a float64 rescale on the library's side
    stay inside ten spacings, and the integer resize underneath is exact -- a larger miss is a bug"""
    from imagdressing_amd.image import DeviceImageProcessor
    cases = [clip_case(golden, j) for j in range(2)]
    got = DeviceImageProcessor("cuda", torch.float32).clip_preprocess([c[0] for c in cases])
    assert got.shape == (2, 3, 224, 224) and got.dtype == torch.float32
    for j, (_, rows, want) in enumerate(cases):
        diff = np.abs(got[j].cpu().numpy()[:, rows, :] - want).max()
        print(f"clip case {j}: max |diff| = {diff:.3e}")
        assert diff <= 1e-5
    half = DeviceImageProcessor("cuda", torch.float16).clip_preprocess(cases[0][0])
    assert half.dtype == torch.float16 and torch.equal(half, got[:1].half())


def host_pack(x):
    """the operations of PipelineBase._decode on the decoder's output, NHWC"""
    image = (x[..., :3].float().cpu() / 2 + 0.5).clamp(0, 1)
    return (image.numpy() * 255).round().astype("uint8")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_pack_u8_every_16_bit_value(golden, dtype):
    """every finite value in [-1.5, 1.5] in each of the three channels: all ties of the rounding and both clamps"""
    from imagdressing_amd import ops
    allv = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = allv[torch.isfinite(allv.float()) & (allv.float().abs() <= 1.5)]
    assert v.numel() > 30000 and (v.float() == 1.5).any() and (v.float() == -1.5).any()
    W = 64
    n = (v.numel() + W - 1) // W * W
    v = torch.cat([v, torch.zeros(n - v.numel(), dtype=dtype)])
    x = torch.full((1, n // W, W, 4), 7.0, dtype=dtype)
    x[0, :, :, 0], x[0, :, :, 1], x[0, :, :, 2] = v.view(-1, W), v.flip(0).view(-1, W), v.roll(n // 3).view(-1, W)
    got = ops.image_pack_u8(x.cuda())
    assert got.shape == (1, n // W, W, 3) and got.dtype == torch.uint8
    want = host_pack(x)
    assert want.min() == 0 and want.max() == 255 and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_pack_u8_ld8(golden, dtype):
    from imagdressing_amd import ops
    x = (torch.randn(2, 24, 40, 8, generator=torch.Generator().manual_seed(4)) * 0.8).to(dtype)
    assert np.array_equal(ops.image_pack_u8(x.cuda()).cpu().numpy(), host_pack(x))


# ---- pipelines ----
def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def pil_noise(seed, w, h, mode="RGB"):
    from PIL import Image
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w) + ((3,) if mode == "RGB" else ()), dtype=np.uint8)
    return Image.fromarray(a)


@pytest.fixture(scope="module")
def engines(golden):
    from imagdressing_amd.vae import AutoencoderKL
    from tests.harness import SMALL, build_pair
    from tests.test_vae_gpu import SMALL as VSMALL
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=torch.float16)
    p["vae"] = AutoencoderKL.random_init(seed=5, config=VSMALL, device="cuda", dtype=torch.float16)
    return p


def sched():
    from imagdressing_amd.scheduler import DDIMScheduler
    return DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                         clip_sample=False, set_alpha_to_one=False, steps_offset=1)


def common_kwargs(R):
    return dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=3,
                guidance_scale=[5.0, 7.0][:R] if R > 1 else 5.0,
                prompt_embeds=torch.cat([rnd(10 + r, 1, 77, 64, scale=0.5) for r in range(R)]).cuda(),
                negative_prompt_embeds=torch.cat([rnd(20 + r, 1, 77, 64, scale=0.5) for r in range(R)]).cuda(),
                ref_clip_hidden_states=torch.cat([rnd(30 + r, 1, 16, 64, scale=0.5) for r in range(R)]).cuda(),
                ref_image_latents=torch.cat([rnd(40 + r, 1, 4, 16, 16) for r in range(R)]).cuda(),
                latents=torch.cat([rnd(50 + r, 1, 4, 16, 16) for r in range(R)]).cuda())


def on_and_off(pipe, call):
    """call() with the default route, with device image I/O, and after switching it off again -> (default, device, default again,
    counter deltas of the three calls)"""
    from imagdressing_amd import ops
    outs, deltas = [], []
    for flag in (False, True, False):
        pipe.enable_device_image_io() if flag else pipe.disable_device_image_io()
        before = dict(ops.IMAGE_IO_COUNTER)
        outs.append(call())
        deltas.append({k: ops.IMAGE_IO_COUNTER[k] - before[k] for k in before})
    return outs, deltas


@torch.no_grad()
def test_controlnet_pipeline_bit_identical(engines):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    p = engines
    pipe = IMAGDressing_v1(vae=p["vae"], reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=sched())
    pose = pil_noise(1, 150, 111)
    (a, b, c), deltas = on_and_off(pipe, lambda: pipe(pose_image=pose, controlnet_conditioning_scale=0.8, output_type="np",
                                                      **common_kwargs(1)).images)
    assert a.shape == (1, 128, 128, 3) and a.dtype == np.uint8 and a.std() > 1
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert deltas[1]["resample"] == 1 and deltas[1]["pack_u8"] == 1                        # the pose image and the decoded batch
    assert not any(deltas[0].values()) and not any(deltas[2].values())                     # ... and the default route before and after
    (pa, pb, _), _ = on_and_off(pipe, lambda: pipe(pose_image=pose, controlnet_conditioning_scale=0.8, output_type="pil",
                                                   **common_kwargs(1)).images)
    assert len(pa) == len(pb) == 1 and pa[0].size == pb[0].size == (128, 128) and pa[0].mode == pb[0].mode == "RGB"
    assert pa[0].tobytes() == pb[0].tobytes() == a[0].tobytes()


@torch.no_grad()
def test_inpainting_pipeline_bit_identical(engines):
    from PIL import Image
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    p = engines
    pipe = IMAGDressing_v1(vae=p["vae"], reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=sched())
    m = np.random.default_rng(9).integers(100, 156, size=(111, 150), dtype=np.uint8)       # grey levels on both sides of the threshold
    m[30:80, 40:110] = 255
    for mask in (Image.fromarray(m), Image.fromarray(np.stack([m, 255 - m, m], -1))):

        def call():
            return pipe(image=pil_noise(2, 150, 111), mask_image=mask, control_image=pil_noise(3, 150, 111), output_type="np",
                        generator=torch.Generator().manual_seed(7), **common_kwargs(1)).images
        (a, b, c), deltas = on_and_off(pipe, call)
        assert a.shape == (1, 128, 128, 3) and a.std() > 1
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert deltas[1]["resample"] == 3 and deltas[1]["pack_u8"] == 1                    # person image, mask, control image
        assert not any(deltas[0].values()) and not any(deltas[2].values())


@torch.no_grad()
def test_request_batched_call_with_images_of_differing_size(engines):
    """R = 2 pose images of different source sizes -> two resample launches into one batch; VAE slicing honoured"""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    p = engines
    pipe = IMAGDressing_v1(vae=p["vae"], reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=sched())
    poses = [pil_noise(4, 150, 111), pil_noise(5, 97, 131)]
    for slicing in (False, True):
        pipe.enable_vae_slicing() if slicing else pipe.disable_vae_slicing()
        try:
            (a, b, c), deltas = on_and_off(pipe, lambda: pipe(pose_image=poses, controlnet_conditioning_scale=[0.8, 0.8], output_type="np",
                                                              **common_kwargs(2)).images)
        finally:
            pipe.disable_vae_slicing()
        assert a.shape == (2, 128, 128, 3) and np.abs(a[0].astype(int) - a[1].astype(int)).max() > 0
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert deltas[1]["resample"] == 2 and deltas[1]["pack_u8"] == (2 if slicing else 1)
        assert not any(deltas[0].values()) and not any(deltas[2].values())
