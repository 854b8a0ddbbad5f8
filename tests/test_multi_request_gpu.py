"""Request-batched pipeline calls on the GPU: R distinct (garment, prompt, latent, guidance, image_scale) requests in ONE call
against R independent runs of the reference loop (oracle.pipeline.denoise at batch 1), and the per-row fused DDIM step
(imd_ddim_cfg_step_rows) against an fp64 statement of the step."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair, err_stats  # noqa: E402

R3_GUIDANCE = (5.0, 7.5, 9.0)
R3_IMAGE_SCALE = (1.0, 0.6, 1.3)


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _sched():
    from imagdressing_amd.scheduler import DDIMScheduler
    return DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                         clip_sample=False, set_alpha_to_one=False, steps_offset=1)


def _bar_small(dtype):
    """the bars of test_pipeline_small_20_steps, relative to the oracle's final latent scale -- except fp16's worst element: 1.5e-2
    instead of 1e-2, because a SOLO call of request 1 here (the single-request path, guidance 7.5, image_scale 0.6) already lands at
    1.1e-2 x std on this seed (rms 2.1e-3, half the rms bar); the batched rows measured identical to the solo calls"""
    return dict(max_abs=1.5e-2, rel_rms=4e-3) if dtype == torch.float16 else dict(max_abs=1e-1, rel_rms=2.5e-2)


def _traj_bar(dtype):
    """the bars of the ControlNet / inpainting / IP-Adapter pipeline tests (test_e2e_gpu._traj_bar)"""
    return dict(max_abs=2e-2, rel_rms=4e-3) if dtype == torch.float16 else dict(max_abs=0.15, rel_rms=2.5e-2)


def _check(out, ref, bar, floor=0.0):
    st = err_stats(out, ref)
    assert torch.isfinite(out).all()
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], floor) and st["rel_rms"] < bar["rel_rms"], st
    return st


def _set_oracle_image_scale(o_unet, s):
    for name, proc in o_unet.attn_processors.items():
        if name.endswith("attn1.processor"):
            proc.scale = s


class _Requests:
    """three requests: garment r (tokens + latents), prompt / negative r, latent seeds, guidance r, image_scale r"""

    def __init__(self, R=3, hw=16, dim=64):
        self.R = R
        self.pe = [g(10 + 10 * r, 1, 77, dim, scale=0.5) for r in range(R)]
        self.ne = [g(11 + 10 * r, 1, 77, dim, scale=0.5) for r in range(R)]
        self.cloth = [g(12 + 10 * r, 2, 16, dim, scale=0.5) for r in range(R)]
        self.refl = [g(13 + 10 * r, 1, 4, hw, hw) for r in range(R)]
        self.hw = hw

    def latent(self, r, i=0):
        return torch.randn(1, 4, self.hw, self.hw, generator=torch.Generator().manual_seed(42 + 100 * r + i))

    def call_kwargs(self, n=1, guidance=R3_GUIDANCE, image_scale=R3_IMAGE_SCALE):
        lat = torch.cat([self.latent(r, i) for r in range(self.R) for i in range(n)])
        return dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=8 * self.hw, height=8 * self.hw,
                    guidance_scale=list(guidance[:self.R]), image_scale=list(image_scale[:self.R]), num_images_per_prompt=n,
                    prompt_embeds=torch.cat(self.pe).cuda(), negative_prompt_embeds=torch.cat(self.ne).cuda(),
                    ref_clip_hidden_states=torch.cat([c[1:2] for c in self.cloth]).cuda(), ref_image_latents=torch.cat(self.refl).cuda(),
                    latents=lat.cuda(), output_type="latent")

    def solo_kwargs(self, r, n=1, guidance=R3_GUIDANCE, image_scale=R3_IMAGE_SCALE):
        lat = torch.cat([self.latent(r, i) for i in range(n)])
        return dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=8 * self.hw, height=8 * self.hw,
                    guidance_scale=guidance[r], image_scale=image_scale[r], num_images_per_prompt=n, prompt_embeds=self.pe[r].cuda(),
                    negative_prompt_embeds=self.ne[r].cuda(), ref_clip_hidden_states=self.cloth[r][1:2].cuda(),
                    ref_image_latents=self.refl[r].cuda(), latents=lat.cuda(), output_type="latent")


_ORACLE = {}


def _oracle(p, reqs, r, i, steps):
    """oracle.pipeline.denoise for image i of request r (batch 1, the request's own garment / prompt / guidance / image_scale)"""
    key = (p["dtype"], r, i, steps)
    if key not in _ORACLE:
        from oracle.ddim import DDIMOracle
        from oracle.pipeline import denoise
        _set_oracle_image_scale(p["o_unet"], R3_IMAGE_SCALE[r])
        try:
            _ORACLE[key] = denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r, i), reqs.pe[r], reqs.ne[r], reqs.cloth[r],
                                   reqs.refl[r], steps, R3_GUIDANCE[r])
        finally:
            _set_oracle_image_scale(p["o_unet"], 1.0)
    return _ORACLE[key]


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def small_pair(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=0, dtype=request.param)
    p["dtype"] = request.param
    return p


def _base_pipe(p):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    return IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           image_encoder=None, ImgProj=lambda h: h, scheduler=_sched(), safety_checker=None, feature_extractor=None)


@torch.no_grad()
def test_three_requests_match_oracle(small_pair):
    """R = 3 distinct garments, prompts, latents, guidance scales and image scales in one call == three reference-loop runs."""
    p, reqs = small_pair, _Requests()
    out = _base_pipe(p)(num_inference_steps=20, **reqs.call_kwargs()).images
    assert out.shape == (3, 4, 16, 16)
    for r in range(3):
        _check(out[r:r + 1], _oracle(p, reqs, r, 0, 20), _bar_small(p["dtype"]))


@torch.no_grad()
def test_three_requests_two_images_each(small_pair):
    """num_images_per_prompt = 2: rows are request-major (request r owns rows 2r, 2r + 1) and every row matches its own oracle run."""
    p, reqs = small_pair, _Requests()
    out = _base_pipe(p)(num_inference_steps=20, **reqs.call_kwargs(n=2)).images
    assert out.shape == (6, 4, 16, 16)
    for r in range(3):
        for i in range(2):
            _check(out[2 * r + i:2 * r + i + 1], _oracle(p, reqs, r, i, 20), _bar_small(p["dtype"]))


@torch.no_grad()
def test_batched_matches_solo_calls(small_pair):
    """each request's rows of the batched call match a solo call of that request (not bit-identical: tile configs depend on the row
    count) within the oracle bars."""
    p, reqs = small_pair, _Requests()
    pipe = _base_pipe(p)
    out = pipe(num_inference_steps=12, **reqs.call_kwargs(n=2)).images
    for r in range(3):
        solo = pipe(num_inference_steps=12, **reqs.solo_kwargs(r, n=2)).images
        _check(out[2 * r:2 * r + 2], solo, _bar_small(p["dtype"]))


@torch.no_grad()
def test_garment_pairing_same_with_and_without_pair_attention(small_pair, monkeypatch):
    """The first hybrid block of the CFG batch (pair-half launch, IMD_CFG_PAIR_ATTN) and every other block pair cond row b with the same
    garment: R = 2 distinct garments give the same result with the de-duplicated first block on and off.  32 x 32 latents, so that the
    level-0 attention qualifies for the duplicated first-phase store (N >= 512)."""
    from imagdressing_amd import ops
    p, reqs = small_pair, _Requests(R=2, hw=32)
    pipe = _base_pipe(p)
    seen = []
    monkeypatch.setattr(ops, "ATTN_EVENT_HOOK", {"match": lambda **kw: (seen.append((kw["B"], kw["N"], kw["L2"])) or False), "events": []})
    monkeypatch.setattr(ops, "CFG_PAIR_ATTN", True)
    a = pipe(num_inference_steps=6, **reqs.call_kwargs()).images
    assert (2, 1024, 1024) in seen                    # the pair-half launch ran: 2 cond rows, garment key set present
    seen.clear()
    monkeypatch.setattr(ops, "CFG_PAIR_ATTN", False)
    b = pipe(num_inference_steps=6, **reqs.call_kwargs()).images
    assert (2, 1024, 1024) not in seen and (4, 1024, 1024) in seen
    bar = 4e-2 if p["dtype"] == torch.bfloat16 else 6e-3
    for r in range(2):
        d = (a[r] - b[r]).pow(2).mean().sqrt() / b[r].pow(2).mean().sqrt()
        assert d < bar, (r, d.item())
    # and the two requests really are different (distinct garments / prompts)
    assert (a[0] - a[1]).pow(2).mean().sqrt() > 10 * bar * a[1].pow(2).mean().sqrt()


@torch.no_grad()
def test_step_graph_replay_of_mixed_guidance_is_bit_identical(small_pair):
    """enable_step_graph: the captured step reads the per-row guidance array at every replay -- bit-identical to the eager loop."""
    p, reqs = small_pair, _Requests()
    pipe = _base_pipe(p)
    pipe.enable_step_graph(False)
    eager = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
    pipe.enable_step_graph(True)
    try:
        g1 = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
        assert getattr(pipe, "_last_step_graph", None) is not None
        g2 = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
    finally:
        pipe.enable_step_graph(False)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, g1) and torch.equal(eager, g2), (eager - g1).abs().max().item()


# ---- ControlNet, inpainting and IP-Adapter pipelines: R = 2 with per-request control / mask / face inputs ----
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_controlnet_two_requests(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dtype)
    reqs, steps, gs = _Requests(R=2), 8, (5.0, 7.0)           # (the guidance values of the single-request pipeline tests)
    pose = [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r)) for r in range(2)]
    refs = torch.cat([denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r), reqs.pe[r], reqs.ne[r], reqs.cloth[r], reqs.refl[r],
                              steps, gs[r], controlnet=p["o_ctrl"], control_image=pose[r], prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]),
                              conditioning_scale=0.8) for r in range(2)])
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    kw = reqs.call_kwargs(guidance=gs, image_scale=(1.0, 1.0))
    out = pipe(num_inference_steps=steps, pose_image=torch.cat(pose).cuda(), controlnet_conditioning_scale=[0.8, 0.8], **kw).images
    for r in range(2):
        _check(out[r:r + 1], refs[r:r + 1], _traj_bar(dtype), floor=1.0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_inpainting_two_requests_strength(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dtype)
    steps, gs, strength = 10, (5.0, 7.0), 0.6
    R = 2
    pe = [g(10 + r, 1, 77, 64, scale=0.5) for r in range(R)]
    ne = [g(20 + r, 1, 77, 64, scale=0.5) for r in range(R)]
    cloth = [g(30 + r, 2, 16, 64, scale=0.5) for r in range(R)]
    refl = [g(40 + r, 1, 4, 16, 16) for r in range(R)]
    img_lat = [g(50 + r, 1, 4, 16, 24) for r in range(R)]
    noise = [g(60 + r, 1, 4, 16, 24) for r in range(R)]
    mask = [torch.zeros(1, 1, 16, 24) for _ in range(R)]
    mask[0][:, :, 4:12, 6:18] = 1.0
    mask[1][:, :, 2:14, 3:10] = 1.0
    ctrl = [torch.rand(1, 3, 128, 192, generator=torch.Generator().manual_seed(70 + r)) for r in range(R)]
    refs = torch.cat([denoise(p["o_unet"], p["o_ref"], DDIMOracle(), None, pe[r], ne[r], cloth[r], refl[r], steps, gs[r], controlnet=p["o_ctrl"],
                              control_image=ctrl[r], prompt_embeds_control=torch.cat([ne[r], pe[r]]), conditioning_scale=1.0,
                              inpaint=dict(mask=mask[r], image_latents=img_lat[r], noise=noise[r]), strength=strength) for r in range(R)])
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    out = pipe(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=192, height=128, num_inference_steps=steps,
               guidance_scale=list(gs), strength=strength, control_image=torch.cat(ctrl).cuda(), prompt_embeds=torch.cat(pe).cuda(),
               negative_prompt_embeds=torch.cat(ne).cuda(), ref_clip_hidden_states=torch.cat([c[1:2] for c in cloth]).cuda(),
               ref_image_latents=torch.cat(refl).cuda(), image_latents=torch.cat(img_lat).cuda(), mask_latents=torch.cat(mask).cuda(),
               noise=torch.cat(noise).cuda(), output_type="latent").images
    assert out.shape == (2, 4, 16, 24)
    for r in range(R):
        _check(out[r:r + 1], refs[r:r + 1], _traj_bar(dtype), floor=1.0)
        keep = (mask[r] == 0).expand(1, 4, -1, -1)
        assert torch.allclose(out[r:r + 1].cpu()[keep], img_lat[r][keep], atol=1e-5)        # each request keeps ITS person outside ITS mask


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_ipa_controlnet_two_requests_with_faces(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_ipa_controlnet import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    p = build_pair(SMALL, seed=3, kind="ipa", with_controlnet=True, dtype=dtype)
    reqs, steps, gs = _Requests(R=2), 8, (7.0, 5.5)
    face_p = [g(80 + r, 1, 4, 64, scale=0.5) for r in range(2)]
    face_n = [g(90 + r, 1, 4, 64, scale=0.5) for r in range(2)]
    pose = [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r)) for r in range(2)]
    refs = torch.cat([denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r), torch.cat([reqs.pe[r], face_p[r]], 1),
                              torch.cat([reqs.ne[r], face_n[r]], 1), reqs.cloth[r], reqs.refl[r], steps, gs[r], controlnet=p["o_ctrl"],
                              control_image=pose[r], prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]), conditioning_scale=0.8)
                      for r in range(2)])

    class FaceProj:      # image_proj_model stand-in: the face clip hidden states carry the request index (+ r + 1 cond, -(r + 1) uncond)
        def __call__(self, idv, clip):
            idx = clip[:, 0, 0].round().long().tolist()
            return torch.cat([face_p[i - 1] if i > 0 else face_n[-i - 1] for i in idx]).cuda()
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, ip_ckpt=None, scheduler=_sched())
    pipe.image_proj_model = FaceProj()
    fc, fu = torch.zeros(2, 257, 1280), torch.zeros(2, 257, 1280)
    for r in range(2):
        fc[r, 0, 0], fu[r, 0, 0] = r + 1, -(r + 1)
    kw = reqs.call_kwargs(guidance=gs, image_scale=(1.0, 1.0))
    out = pipe(num_inference_steps=steps, pose_image=[pose[0].cuda(), pose[1].cuda()], faceid_embeds=torch.ones(2, 512),
               face_clip_hidden_states=fc, face_uncond_clip_hidden_states=fu, ipa_scale=0.9, s_lora_scale=0.2, c_lora_scale=[0.2, 0.2],
               controlnet_conditioning_scale=0.8, **kw).images
    for r in range(2):
        _check(out[r:r + 1], refs[r:r + 1], _traj_bar(dtype), floor=1.0)


# ---- imd_ddim_cfg_step_rows ----
def _ddim_ref(z, eps, g_rows, a_t, a_prev, mask=None, z_img=None, noise=None, a_next=None, var_noise=None, sigma=0.0):
    """fp64 statement of the fused step (CFG, DDIM, stochastic term, inpaint blend) with one guidance value per latent row"""
    z, eps = z.double(), eps.double()
    B = z.shape[0]
    c, u = eps[:B], eps[B:]
    gg = g_rows.double().view(B, 1, 1)
    e = u + gg * (c - u)
    x0 = (z - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    dir_c = (1 - a_prev) ** 0.5 if var_noise is None else max(1 - a_prev - sigma ** 2, 0.0) ** 0.5
    zn = a_prev ** 0.5 * x0 + dir_c * e
    if var_noise is not None:
        zn = zn + sigma * var_noise.double()
    if mask is not None:
        san, s1n = (1.0, 0.0) if a_next is None else (a_next ** 0.5, (1 - a_next) ** 0.5)
        proper = san * z_img.double() + s1n * noise.double()
        m = mask.double().unsqueeze(-1)
        zn = (1 - m) * proper + m * zn
    return zn


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
@pytest.mark.parametrize("mode", ["host", "coefs", "var_noise"])
@torch.no_grad()
def test_ddim_cfg_step_rows_kernel(dtype, inpaint, mode):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops
    B, HW = 3, 16 * 24
    gen = torch.Generator().manual_seed(7)
    z0 = torch.randn(B, HW, 4, generator=gen)
    eps = torch.randn(2 * B, HW, 4, generator=gen)
    g_rows = torch.tensor([5.0, 7.5, 9.0])
    a_t, a_prev, a_next = 0.42, 0.61, 0.73
    kw = {}
    if inpaint:
        kw = dict(mask=(torch.rand(B, HW, generator=gen) > 0.5).float(), z_img=torch.randn(B, HW, 4, generator=gen),
                  noise=torch.randn(B, HW, 4, generator=gen))
    extra = {}
    if mode == "var_noise":
        extra = dict(var_noise=torch.randn(B, HW, 4, generator=gen), sigma=0.17)
    ref = _ddim_ref(z0, eps, g_rows, a_t, a_prev, a_next=a_next if inpaint else None, **kw, **extra)

    def run(guidance):
        z = z0.clone().cuda()
        x_next = torch.full((2 * B, HW, 8), 7.0, dtype=dtype, device="cuda")
        dkw = {k: v.cuda() for k, v in kw.items()}
        dkw.update({k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in extra.items()})
        if mode == "coefs":
            coefs = torch.tensor(ops.ddim_coefs(a_t, a_prev, a_next if inpaint else None), dtype=torch.float32, device="cuda")
            ops.ddim_cfg_step(z, eps.cuda(), x_next, guidance=guidance, coefs=coefs, **dkw)
        else:
            ops.ddim_cfg_step(z, eps.cuda(), x_next, guidance=guidance, a_t=a_t, a_prev=a_prev,
                              a_next=a_next if inpaint else None, **dkw)
        torch.cuda.synchronize()
        return z.cpu(), x_next.cpu()

    z, x_next = run(g_rows.cuda())
    assert (z.double() - ref).abs().max().item() < 1e-4 * max(ref.abs().max().item(), 1.0)
    for half in (x_next[:B], x_next[B:]):            # the next UNet input, both CFG halves, channels 4..7 zero
        assert torch.equal(half[..., :4], z.to(dtype)) and not half[..., 4:].any()
    # a uniform guidance array is bit-identical to the scalar entry point
    zs, xs = run(7.5)
    zr, xr = run(torch.full((B,), 7.5).cuda())
    assert torch.equal(zs, zr) and torch.equal(xs, xr)
    # per-row: row b of the mixed call equals the scalar step with guidance g[b] (bitwise: same arithmetic per element)
    for b in range(B):
        zb, _ = run(float(g_rows[b]))
        assert torch.equal(zb[b], z[b]), b
