"""``soft_mask`` of the inpainting pipeline on the GPU (small synthetic engines, 64 x 64 images = 8 x 8 latents, 6 steps).  Everything the
feature adds is integer work and 0 / 1 masks, so the comparisons are ``torch.equal``: an aligned binary mask gives the hard call, a
three-level mask gives one hard call up to the gray level's release and another from there, graph replay is eager, a hard request keeps
its bits beside a soft one, the two image routes agree, ``strength`` < 1 counts the executed positions, and the default changes
neither a bit nor a library call."""
import numpy as np
import pytest
import torch

from tests.inpaint_cases import noise_image
from tests.soft_mask_cases import aligned_binary_mask, three_level_mask
from tests.test_mask_blur_pipeline_gpu import Recorder

pytestmark = pytest.mark.gpu

SIZE, LAT, STEPS, GS = (64, 64), (8, 8), 6, 5.0
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def scheduler(name):
    from imagdressing_amd import scheduler as S
    return {"ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW),
            "dpm": lambda: S.DPMSolverMultistepScheduler(**KW), "euler": lambda: S.EulerDiscreteScheduler(**KW),
            "euler_a": lambda: S.EulerAncestralDiscreteScheduler(**KW),
            "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW),
            "unipc": lambda: S.UniPCMultistepScheduler(fused_step=True, **KW)}[name]()


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
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=scheduler("ddim"))


def pil(a):
    from PIL import Image
    return Image.fromarray(a)


def call(pipe, R=1, sched="ddim", **over):
    """latents out; the person image comes as latents and the ControlNet image as a tensor unless a test says otherwise"""
    pipe.scheduler = scheduler(sched)
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=SIZE[1], height=SIZE[0], num_inference_steps=STEPS,
              guidance_scale=GS, prompt_embeds=torch.cat([g(10 + r, 1, 77, 64, scale=0.5) for r in range(R)]).cuda(),
              negative_prompt_embeds=torch.cat([g(20 + r, 1, 77, 64, scale=0.5) for r in range(R)]).cuda(),
              ref_clip_hidden_states=g(12, 2, 16, 64, scale=0.5)[1:2].cuda(), ref_image_latents=g(13, 1, 4, 16, 16).cuda(),
              control_image=torch.rand(1, 3, *SIZE, generator=torch.Generator().manual_seed(18)).cuda(),
              image_latents=g(17, 1, 4, *LAT).cuda(), noise=g(42, R, 4, *LAT).cuda(), output_type="latent")
    kw.update(over)
    return pipe(**kw).images


def spy_denoise(pipe, seen):
    """``pipe.denoise`` recording its keywords (the release map, everything a restart needs) -> the undo"""
    real = pipe.denoise

    def spy(**kw):
        seen.append(kw)
        return real(**kw)
    pipe.denoise = spy
    return lambda: pipe.__dict__.pop("denoise")


ON = np.random.default_rng(3).random(LAT) < 0.5
BINARY = aligned_binary_mask(SIZE, LAT, ON)
GRAY = 128                                                        # ceil(128 / 255 * 6) = 4 free steps: release 2
THREE, LEVEL = three_level_mask(SIZE, LAT, GRAY)


# ---- 1. an aligned binary mask is the hard call ----
@pytest.mark.parametrize("device_io", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sched", ["ddim", "dpm", "euler", "pndm", "unipc"])
@torch.no_grad()
def test_aligned_binary_mask_equals_the_hard_call(pipe, sched, device_io):
    from imagdressing_amd import ops
    pipe.enable_device_image_io(device_io)
    try:
        hard = call(pipe, sched=sched, mask_image=pil(BINARY), soft_mask=False)
        before = dict(ops.SOFT_MASK_COUNTER)
        soft = call(pipe, sched=sched, mask_image=pil(BINARY), soft_mask=True)
    finally:
        pipe.disable_device_image_io()
    assert torch.isfinite(hard).all() and torch.equal(soft, hard)
    calls = STEPS + 1 if sched == "pndm" else STEPS
    assert ops.SOFT_MASK_COUNTER["soft_mask_rows"] - before["soft_mask_rows"] == calls          # the launches were made
    assert ops.SOFT_MASK_COUNTER["mask_release"] - before["mask_release"] == (1 if device_io else 0)
    keep = torch.from_numpy(~ON)[None, None].expand(1, 4, -1, -1)
    assert torch.allclose(soft.cpu()[keep], g(17, 1, 4, *LAT)[keep], atol=1e-5)          # outside the mask: the clean original


# ---- 2. three levels: two hard calls, joined at the release step ----
def nchw(z):
    return z.view(z.shape[0], *LAT, 4).permute(0, 3, 1, 2).contiguous()


@torch.no_grad()
def test_three_level_mask_is_two_hard_calls(pipe):
    from imagdressing_amd.image import mask_release_reference
    release = int(mask_release_reference(THREE, *LAT, STEPS)[LEVEL == 1][0])
    assert release == 2 == STEPS - -(-GRAY * STEPS // 255)
    level = torch.from_numpy(LEVEL)
    full = (level == 2).float()[None, None].cuda()                # [c == 1]
    any_ = (level > 0).float()[None, None].cuda()                 # [c > 0]
    seen, tr, tr_full = [], [], []
    undo = spy_denoise(pipe, seen)
    try:
        out = call(pipe, mask_image=pil(THREE), soft_mask=True, trace=tr)
    finally:
        undo()
    call(pipe, mask_latents=full, trace=tr_full)
    assert len(tr) == len(tr_full) == STEPS
    for k in range(release):                                      # the gray band is reset like an unmasked pixel
        assert torch.equal(tr[k], tr_full[k]), k
    assert not torch.equal(tr[release], tr_full[release])
    # from there the gray band is free: the hard call with [c > 0], restarted from the state before the release step
    kw = dict(seen[0])
    inpaint = {k: v for k, v in kw["inpaint"].items() if k not in ("release", "soft_rows")}
    tr_any = []
    kw.update(latents=nchw(tr[release - 1]), t_start=release, inpaint=dict(inpaint, mask=any_), trace=tr_any)
    pipe.scheduler = scheduler("ddim")
    rest = pipe.denoise(**kw)
    assert len(tr_any) == STEPS - release
    for k in range(release, STEPS):
        assert torch.equal(tr[k], tr_any[k - release]), k
    assert torch.equal(rest, out)
    # a gray pixel before its release IS the re-noised original: b_img z_img + b_noise noise of the position the blend aims at
    sch = scheduler("ddim")
    sch.set_timesteps(STEPS)
    ts = [int(t) for t in sch.timesteps]
    z_img = g(17, 1, 4, *LAT).permute(0, 2, 3, 1).reshape(1, -1, 4).double()
    noise = g(42, 1, 4, *LAT).permute(0, 2, 3, 1).reshape(1, -1, 4).double()
    gray = (level == 1).reshape(-1)
    for k in range(release):
        a = float(sch.alpha(ts[k + 1]))
        t1, t2 = a ** 0.5 * z_img, (1.0 - a) ** 0.5 * noise
        err = (tr[k].cpu().double() - (t1 + t2)).abs()[:, gray]
        bound = 2.0 ** -22 * (t1.abs() + t2.abs())[:, gray]
        print(f"gray pixels after step {k}: max err / bound = {(err / bound).max().item():.3f}")
        assert (err <= bound).all()
    free = (tr[STEPS - 1].cpu().double() - z_img).abs()[:, gray]
    assert free.max() > 1e-2                                      # ... and is repainted afterwards
    zero = (level == 0).reshape(-1)
    assert torch.allclose(tr[STEPS - 1].cpu()[:, zero], z_img.float()[:, zero], atol=1e-5)          # c = 0 ends as the clean original


# ---- 3. graph replay ----
@pytest.mark.parametrize("sched", ["ddim", "dpm"])
@torch.no_grad()
def test_step_graph_is_bit_identical_to_eager(pipe, sched):
    eager = call(pipe, sched=sched, mask_image=pil(THREE), soft_mask=True)
    pipe.__dict__.pop("_last_step_graph", None)
    pipe.enable_step_graph()
    try:
        replayed = call(pipe, sched=sched, mask_image=pil(THREE), soft_mask=True)
        assert "_last_step_graph" in pipe.__dict__                # (the call did replay)
    finally:
        pipe.enable_step_graph(False)
    assert torch.equal(replayed, eager)
    assert not torch.equal(eager, call(pipe, sched=sched, mask_image=pil(THREE)))          # and the keyword is seen in the result


# ---- 4. a hard request beside a soft one ----
@torch.no_grad()
def test_hard_request_keeps_its_bits_beside_a_soft_one(pipe):
    kw = dict(R=2, sched="dpm", mask_image=pil(THREE), guidance_scale=[5.0, 7.0])
    both_hard = call(pipe, soft_mask=[False, False], **kw)
    mixed = call(pipe, soft_mask=[False, True], **kw)
    assert torch.equal(mixed[0], both_hard[0]) and not torch.equal(mixed[1], both_hard[1])
    both_soft = call(pipe, soft_mask=True, **kw)
    assert torch.equal(mixed[1], both_soft[1])                    # and the soft one does not depend on its neighbour
    two = call(pipe, soft_mask=[False, True], num_images_per_prompt=2, noise=g(43, 4, 4, *LAT).cuda(), **kw)
    hard2 = call(pipe, soft_mask=False, num_images_per_prompt=2, noise=g(43, 4, 4, *LAT).cuda(), **kw)
    assert torch.equal(two[:2], hard2[:2]) and not torch.equal(two[2], hard2[2]) and not torch.equal(two[3], hard2[3])


# ---- 5. the two image routes ----
@pytest.mark.parametrize("extra", [dict(), dict(mask_blur=4), dict(mask_blur=4, padding_mask_crop=16, control_image=None, image_latents=None)],
                         ids=["plain", "blur", "blur_crop"])
@torch.no_grad()
def test_host_and_device_routes_agree(pipe, extra):
    from imagdressing_amd.image import get_crop_region, mask_filter_host, mask_release_reference
    big = (111, 150)                                              # the person image: neither axis a multiple of the latent
    m = np.zeros(big, np.uint8)
    m[30:80, 40:110] = np.linspace(40, 255, 70).astype(np.uint8)[None]
    kw = dict(mask_image=pil(m), soft_mask=True, image=pil(noise_image(2, big)), **extra)
    outs, maps = [], []
    for flag in (False, True):
        seen = []
        undo = spy_denoise(pipe, seen)
        pipe.enable_device_image_io(flag)
        try:
            outs.append(call(pipe, generator=torch.Generator().manual_seed(7), **kw))
        finally:
            pipe.disable_device_image_io()
            undo()
        rel = seen[0]["inpaint"]["release"]
        assert rel.dtype == torch.uint16 and rel.is_cuda == flag
        maps.append(rel.cpu().to(torch.int32))
    assert torch.equal(maps[0], maps[1]) and torch.equal(outs[0], outs[1])
    want = m if "mask_blur" not in extra else np.asarray(mask_filter_host(pil(m), 0, 4.0))
    if "padding_mask_crop" in extra:
        x1, y1, x2, y2 = get_crop_region(want, SIZE[1], SIZE[0], pad=16)
        assert (x2 - x1, y2 - y1) != (big[1], big[0])             # (a real window)
        want = np.ascontiguousarray(want[y1:y2, x1:x2])
    assert torch.equal(maps[0][0], torch.from_numpy(mask_release_reference(want, *LAT, STEPS).astype(np.int32)))
    assert len(maps[0].unique()) > 2                              # gray levels are in it


# ---- 6. strength < 1 ----
@torch.no_grad()
def test_strength_counts_the_executed_positions(pipe):
    from imagdressing_amd.image import mask_release_reference
    level = torch.from_numpy(LEVEL)
    seen, tr, tr_full = [], [], []
    undo = spy_denoise(pipe, seen)
    try:
        call(pipe, mask_image=pil(THREE), soft_mask=True, strength=0.5, trace=tr)
    finally:
        undo()
    n = 3                                                         # int(6 * 0.5) positions run
    assert len(tr) == n and seen[0]["t_start"] == STEPS - n
    rel = seen[0]["inpaint"]["release"].cpu().to(torch.int32)
    assert torch.equal(rel[0], torch.from_numpy(mask_release_reference(THREE, *LAT, n).astype(np.int32)))
    release = int(rel[0][level == 1][0])
    assert release == 1 == n - -(-GRAY * n // 255)                # ceil(128 / 255 * 3) = 2 free steps
    call(pipe, mask_latents=(level == 2).float()[None, None].cuda(), strength=0.5, trace=tr_full)
    assert torch.equal(tr[0], tr_full[0]) and not torch.equal(tr[1], tr_full[1])
    zero = (level == 0).reshape(-1)
    z_img = g(17, 1, 4, *LAT).permute(0, 2, 3, 1).reshape(1, -1, 4)
    assert torch.allclose(tr[n - 1].cpu()[:, zero], z_img[:, zero], atol=1e-5)


# ---- 7. the default ----
@pytest.mark.parametrize("device_io", [False, True], ids=["host", "device"])
@torch.no_grad()
def test_absent_and_false_are_the_same_call(pipe, device_io, monkeypatch):
    from collections import Counter
    from imagdressing_amd import _lib
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    pipe.enable_device_image_io(device_io)
    try:
        outs, counts = [], []
        for extra in (dict(), dict(soft_mask=False), dict(soft_mask=[False]), dict(soft_mask=True)):
            rec.calls = []
            outs.append(call(pipe, sched="dpm", mask_image=pil(THREE), **extra))
            counts.append(Counter(rec.calls))
    finally:
        pipe.disable_device_image_io()
    assert sum(counts[0].values()) > 10 and counts[0]["imd_soft_mask_rows"] == 0 and counts[0]["imd_image_mask_release"] == 0
    assert counts[1] == counts[0] and counts[2] == counts[0]
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    added = counts[3] - counts[0]
    assert added == Counter({"imd_soft_mask_rows": STEPS, **({"imd_image_mask_release": 1} if device_io else {})})
    assert not counts[0] - counts[3]                              # nothing else changed
    assert not torch.equal(outs[3], outs[0])


# ---- 8. what it composes with ----
@pytest.mark.parametrize("combo", ["eta", "euler_a_device_noise", "guidance_rescale", "deepcache", "overlay"])
@torch.no_grad()
def test_composes_with_the_other_switches(pipe, combo):
    """under each switch the aligned binary mask still gives the hard call, and the three-level mask something else"""
    kw, undo = {}, lambda: None
    if combo == "eta":
        kw = dict(sched="ddim", eta=0.5, variance_noise=[g(300 + i, 1, 4, *LAT).cuda() for i in range(STEPS)])
    elif combo == "euler_a_device_noise":
        pipe.enable_device_noise()
        undo = pipe.disable_device_noise
        kw = dict(sched="euler_a", noise=None, seed=11)          # the initial noise, the blend's and every step's from the request's seed
    elif combo == "guidance_rescale":
        kw = dict(sched="dpm", guidance_rescale=0.7)
    elif combo == "deepcache":
        pipe.enable_deepcache()
        undo = pipe.disable_deepcache
        kw = dict(sched="dpm")
    else:
        kw = dict(sched="dpm", overlay=True, output_type="np", image=pil(noise_image(2, SIZE)), image_latents=None)

    def run(**over):
        if combo == "overlay":                                    # (the VAE samples the image latents: the same draw in every run)
            over["generator"] = torch.Generator().manual_seed(7)
        out = call(pipe, **kw, **over)
        return torch.from_numpy(out) if isinstance(out, np.ndarray) else out
    try:
        hard = run(mask_image=pil(BINARY))
        soft = run(mask_image=pil(BINARY), soft_mask=True)
        gray_hard = run(mask_image=pil(THREE))
        gray_soft = run(mask_image=pil(THREE), soft_mask=True)
    finally:
        undo()
    assert torch.equal(soft, hard) and not torch.equal(gray_soft, gray_hard)
    assert torch.isfinite(gray_soft.float()).all()


# ---- 9. a caller's float mask_latents ----
@pytest.mark.parametrize("sched", ["ddim", "dpm"])
@torch.no_grad()
def test_float_mask_latents_are_read_never_written(pipe, sched):
    """the levels as an fp32 [1, 1, h, w] tensor on the device reach the loop without a copy: the step launches must write a buffer of
    the loop's own.  Twice the same call with the same tensor: the tensor keeps its bits, the outputs agree, and they are those of the
    mask image with the same three levels"""
    levels = torch.tensor([0.0, GRAY / 255.0, 1.0])[torch.from_numpy(LEVEL)][None, None].cuda().contiguous()
    saved = levels.clone()
    first = call(pipe, sched=sched, mask_latents=levels, soft_mask=True)
    assert torch.equal(levels, saved)
    second = call(pipe, sched=sched, mask_latents=levels, soft_mask=True)
    assert torch.equal(levels, saved) and torch.equal(second, first)
    assert torch.equal(first, call(pipe, sched=sched, mask_image=pil(THREE), soft_mask=True))
    assert not torch.equal(first, call(pipe, sched=sched, mask_latents=(saved > 0).float()))          # (and not the hard call it would decay to)
    # the loop itself, given the tensors directly
    seen = []
    undo = spy_denoise(pipe, seen)
    try:
        call(pipe, sched=sched, mask_latents=levels, soft_mask=True)
    finally:
        undo()
    pipe.scheduler = scheduler(sched)
    assert seen[0]["inpaint"]["mask"].data_ptr() == levels.data_ptr()
    assert torch.equal(pipe.denoise(**seen[0]), first) and torch.equal(levels, saved)
