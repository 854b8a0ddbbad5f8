"""The fused sampler step on the GPU: ``imd_sampler_step`` against an fp64 statement of the step over its shapes and options, and the
four schedulers built on it (DPM-Solver++, Euler, Euler-ancestral, PNDM) through the pipelines -- plumbing against the coefficient
rows applied by hand, trajectories against the reference loop driven by the library-form restatements (tests/sampler_oracle.py),
graph replay, request-batched guidance and the inpainting blend."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair, err_stats  # noqa: E402
from tests.sampler_oracle import DPMSolverOracle, EulerAncestralOracle, EulerOracle, PNDMOracle, apply_row  # noqa: E402

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _mk(name):
    from imagdressing_amd import scheduler as S
    return {"dpm": lambda: S.DPMSolverMultistepScheduler(**KW), "euler": lambda: S.EulerDiscreteScheduler(**KW),
            "euler_a": lambda: S.EulerAncestralDiscreteScheduler(**KW),
            "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW)}[name]()


ORACLES = {"dpm": DPMSolverOracle, "euler": EulerOracle, "euler_a": EulerAncestralOracle, "pndm": PNDMOracle}


# ---- the kernel ----
def _step_ref(z, eps, g_rows, c, H, noise, blend):
    """fp64 statement of imd_sampler_step for one coefficient block c (ops.sampler_coefs order) -> (z', m)"""
    B = z.shape[0]
    gr = g_rows.double().view(B, 1, 1)
    e = eps[B:].double() + gr * (eps[:B].double() - eps[B:].double())
    m = c[0] * z.double() + c[1] * e
    zn = c[2] * z.double() + c[3] * m
    for k in range(H.shape[0]):
        zn = zn + c[4 + k] * H[k].double()
    if noise is not None:
        zn = zn + c[8] * noise.double()
    if blend is not None:
        mask, z_img, bn = (t.double() for t in blend)
        zn = (1 - mask.unsqueeze(-1)) * (c[9] * z_img + c[10] * bn) + mask.unsqueeze(-1) * zn
    return zn, m


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [0, 1, 4])
@pytest.mark.parametrize("B,HW", [(1, 1), (3, 77), (2, 300)], ids=["lone", "partial-block", "row-boundary"])
def test_sampler_step_kernel(B, HW, K, dtype):
    """a lone element, a partial block and a row boundary inside a block; no history, one slot, all four; noise and blend on and off;
    no store and a store into a slot that the same launch reads.  Bar 1e-4 x max(|ref|, 1) (fp32 arithmetic on O(1) data, the bar of
    test_ddim_cfg_step_rows_kernel); everything the kernel only rounds or copies is compared bit for bit."""
    from imagdressing_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z0, eps = g(1, B, HW, 4), g(2, 2 * B, HW, 4)
    H0 = g(3, K, B, HW, 4)
    noise, z_img, bn = g(4, B, HW, 4), g(5, B, HW, 4), g(6, B, HW, 4)
    mask = (torch.rand(B, HW, generator=torch.Generator().manual_seed(7)) > 0.4).float()
    mask[0, 0] = 0.25                                     # a fractional value too
    g_mixed = torch.tensor([5.0, 7.5, 9.0][:B])
    zh = [0.7, -0.3, 0.45, -0.2][:K]
    for use_noise in (False, True):
        for use_blend in (False, True):
            for store in ([-1] if K == 0 else [-1, 0]):
                c = ops.sampler_coefs(m_x=1.2, m_e=-0.8, z_x=0.9, z_m=0.35, z_h=zh, z_n=0.6, b_img=0.95, b_noise=0.3, in_scale=0.37, store=store)
                what = (B, HW, K, use_noise, use_blend, store)
                blend = (mask, z_img, bn) if use_blend else None
                ref, m_ref = _step_ref(z0, eps, g_mixed, c, H0, noise if use_noise else None, blend)

                def run(guidance, coefs):
                    z, H, xn = z0.clone().cuda(), (H0.clone().cuda() if K else None), torch.full((2 * B, HW, 8), 7.0, dtype=dtype).cuda()
                    kw = dict(mask=mask.cuda(), z_img=z_img.cuda(), blend_noise=bn.cuda()) if use_blend else {}
                    ops.sampler_step(z, eps.cuda(), xn, guidance=guidance, coefs=coefs, hist=H, noise=noise.cuda() if use_noise else None, **kw)
                    return z, H, xn
                z, H, xn = run(g_mixed.cuda(), c)
                bar = 1e-4 * max(ref.abs().max().item(), 1.0)
                assert (z.double().cpu() - ref).abs().max().item() < bar, what
                # the next UNet input: the 16-bit rounding of in_scale z' exactly, padded channels zero, both halves the same registers
                c32 = torch.tensor(c, dtype=torch.float32)
                assert torch.equal(xn[:B, :, :4], (z * c32[11].cuda()).to(dtype)), what
                assert torch.equal(xn[:B], xn[B:]) and not xn[..., 4:].any(), what
                for k in range(K):
                    if k == store:
                        assert (H[k].double().cpu() - m_ref).abs().max().item() < 1e-4 * max(m_ref.abs().max().item(), 1.0), what
                    else:
                        assert torch.equal(H[k].cpu(), H0[k]), what
                # the coefficient block read from device memory: the same bits
                zd, Hd, xd = run(g_mixed.cuda(), c32.cuda())
                assert torch.equal(zd, z) and torch.equal(xd, xn) and (K == 0 or torch.equal(Hd, H)), what
                # per-row guidance: a uniform array == the scalar form; row b of the mixed call == the scalar call with g[b]
                zs, Hs, xs = run(7.5, c)
                zu, Hu, xu = run(torch.full((B,), 7.5).cuda(), c)
                assert torch.equal(zs, zu) and torch.equal(xs, xu) and (K == 0 or torch.equal(Hs, Hu)), what
                for b in range(B):
                    zb, Hb, xb = run(float(g_mixed[b]), c)
                    assert torch.equal(zb[b], z[b]) and torch.equal(xb[b], xn[b]) and torch.equal(xb[B + b], xn[B + b]), (what, b)
                    assert K == 0 or torch.equal(Hb[:, b], H[:, b]), (what, b)
    # without x_next (the schedulers' tensor surface): same latent
    z = z0.clone().cuda()
    ops.sampler_step(z, eps.cuda(), None, guidance=7.5, coefs=ops.sampler_coefs(z_h=zh, m_x=1.2, z_m=0.35), hist=H0.clone().cuda() if K else None)
    assert torch.isfinite(z).all()


def test_sampler_step_launcher_refusals():
    """errors, and nothing launched: the latent keeps its bits"""
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    B, HW = 2, 40
    z0 = g(1, B, HW, 4).cuda()
    eps, xn = g(2, 2 * B, HW, 4).cuda(), torch.zeros(2 * B, HW, 8, dtype=torch.float16).cuda()
    c = ops.sampler_coefs
    buf = torch.zeros(B * HW * 4 + 4).cuda()
    off = buf[1:1 + B * HW * 4].view(B, HW, 4)                                      # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    cases = [(dict(hist=torch.zeros(5, B, HW, 4).cuda()), c(), "K (5)"),
             (dict(hist=torch.zeros(2, B, HW, 4).cuda()), c(store=2), "store slot 2"),
             (dict(), c(store=0), "store slot 0"),
             (dict(hist=torch.zeros(2, B, HW, 4).cuda()), c(store=-2), "store slot -2"),
             (dict(mask=torch.ones(B, HW).cuda()), c(), "inpaint mask"),
             (dict(mask=torch.ones(B, HW).cuda(), z_img=z0.clone()), c(), "inpaint mask"),
             (dict(mask=torch.ones(B, HW).cuda(), blend_noise=z0.clone()), c(), "inpaint mask"),
             (dict(noise=off), c(), "16-byte"), (dict(hist=off), c(), "16-byte"),
             (dict(mask=torch.ones(B, HW).cuda(), z_img=off, blend_noise=z0.clone()), c(), "16-byte")]
    for kw, coefs, word in cases:
        z = z0.clone()
        with pytest.raises(ImdError, match=word.replace("(", r"\(").replace(")", r"\)")):
            ops.sampler_step(z, eps, xn, guidance=7.5, coefs=coefs, **kw)
        assert torch.equal(z, z0) and not xn.any(), word
    with pytest.raises(ImdError, match="16-byte"):
        ops.sampler_step(off, eps, xn, guidance=7.5, coefs=c())
    with pytest.raises(ImdError, match="13"):
        ops.sampler_step(z0.clone(), eps, xn, guidance=7.5, coefs=[1.0] * 6)
    with pytest.raises(ImdError, match="per-row guidance"):
        ops.sampler_step(z0.clone(), eps, xn, guidance=torch.ones(B + 1).cuda(), coefs=c())


# ---- the schedulers through the pipelines ----
@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def small_pair(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=0, dtype=request.param)
    p["dtype"] = request.param
    return p


def _pipe(p, sch):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    return IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           image_encoder=None, ImgProj=lambda h: h, scheduler=sch, safety_checker=None, feature_extractor=None)


def _call_kw(lat, steps, gs, **over):
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=steps,
              guidance_scale=gs, num_images_per_prompt=lat.shape[0], prompt_embeds=g(10, 1, 77, 64, scale=0.5).cuda(),
              negative_prompt_embeds=g(11, 1, 77, 64, scale=0.5).cuda(), ref_clip_hidden_states=g(12, 2, 16, 64, scale=0.5)[1:2].cuda(),
              ref_image_latents=g(13, 1, 4, 16, 16).cuda(), latents=lat.cuda(), output_type="latent")
    kw.update(over)
    return kw


@pytest.mark.parametrize("name", ["dpm", "euler", "euler_a", "pndm"])
@torch.no_grad()
def test_pipeline_sampler_plumbing_small(name):
    """Each class through the pipeline == its coefficient rows applied by hand in fp64 to the same UNet outputs, at EVERY step (the
    host math is tested on the CPU; this checks the plumbing: CFG, the history slots, the noise, the scaled 16-bit UNet input, the
    unrounded timesteps): step i is recomputed from the pipeline's own state after step i - 1."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.unet import nchw_to_nhwc8
    dt = torch.float16
    p = build_pair(SMALL, seed=0, dtype=dt)
    sch = _mk(name)
    pipe = _pipe(p, sch)
    lat = g(20, 2, 4, 16, 16)
    steps, gs = 6, 7.5
    calls = steps + 1 if name == "pndm" else steps
    vn = [g(300 + i, 2, 4, 16, 16) for i in range(calls)]
    kw = _call_kw(lat, steps, gs, **(dict(variance_noise=[v.cuda() for v in vn]) if name == "euler_a" else {}))
    trace = []
    out = pipe(trace=trace, **kw).images
    assert torch.isfinite(out).all() and len(trace) == calls == sch.steps()
    assert torch.equal(pipe(**kw).images, out)                      # deterministic and restartable
    if name == "pndm":
        assert [int(t) for t in sch.timesteps] == [831, 665, 665, 499, 333, 167, 1]
    if name == "euler":
        assert [round(float(t), 1) for t in sch.timesteps] == [999.0, 799.2, 599.4, 399.6, 199.8, 0.0]
    # by hand: the same UNet, the same inputs
    unet = p["e_unet"]
    p["e_ref"].forward_nhwc(nchw_to_nhwc8(kw["ref_image_latents"], dt), 0, kw["ref_clip_hidden_states"].to(dt).contiguous())
    sa = {n: pr.cache["hidden_states"] for n, pr in p["e_ref"].attn_processors.items()}
    ehs = torch.cat([kw["prompt_embeds"], kw["negative_prompt_embeds"]]).to(dt).contiguous()
    cak = {"sa_hidden_states": sa, "sa_batch_mask": torch.cat([torch.ones(2), torch.zeros(2)]).cuda(), "sa_pair_layout": True}
    ts = [t.item() for t in sch.timesteps]
    unet.precompute_time_embeddings(ts, torch.device("cuda"))        # the rows the loop picked
    try:
        z = (lat.cuda().float() * sch.init_noise_sigma).permute(0, 2, 3, 1).reshape(2, 256, 4).contiguous()
        hist = []
        for i in range(calls):
            scale = torch.tensor(sch.input_scale(i), dtype=torch.float32).cuda()
            x_in = torch.zeros(4, 16, 16, 8, dtype=dt, device="cuda")
            x_in[..., :4] = torch.cat([z, z]).mul(scale).to(dt).view(4, 16, 16, 4)
            eps = unet.forward_nhwc(x_in, ts[i], ehs, cak, None, None, cfg_pair=True).view(4, 256, 4).double()
            e = eps[2:] + gs * (eps[:2] - eps[2:])
            nz = vn[i].cuda().permute(0, 2, 3, 1).reshape(2, 256, 4).double() if name == "euler_a" else None
            want = apply_row(sch.plan(i), z.double(), e, hist, noise=nz)
            assert torch.allclose(trace[i].double(), want, rtol=1e-4, atol=1e-4), (name, i, (trace[i].double() - want).abs().max().item())
            z = trace[i]
    finally:
        unet.clear_time_embeddings()
    assert torch.equal(out, trace[-1].view(2, 16, 16, 4).permute(0, 3, 1, 2))


_ORACLE = {}


def _oracle_run(p, name, lat, steps, gs, vn):
    """oracle.pipeline.denoise driven by the restatement of ``name`` (fp32 CPU oracle: the same for both element types)"""
    if name not in _ORACLE:
        from oracle.pipeline import denoise
        pe, ne = g(10, 1, 77, 64, scale=0.5), g(11, 1, 77, 64, scale=0.5)
        cloth, refl = g(12, 2, 16, 64, scale=0.5), g(13, 1, 4, 16, 16)
        orc = ORACLES[name]()
        orc.set_timesteps(steps)
        extra = dict(eta=1.0, variance_noise=vn) if name == "euler_a" else {}       # (eta only routes the noise list to ``step``)
        _ORACLE[name] = denoise(p["o_unet"], p["o_ref"], orc, lat * orc.init_noise_sigma, pe, ne, cloth, refl, steps, gs, **extra)
    return _ORACLE[name]


@pytest.mark.parametrize("name", ["dpm", "euler", "euler_a", "pndm"])
@torch.no_grad()
def test_pipeline_samplers_10_steps_vs_oracle(small_pair, name):
    """10 steps of each class through the HIP pipeline against the reference loop semantics (oracle/pipeline.py: two B = 1 UNet calls
    per step, custom CFG, the scheduler's own scale_model_input) driven by the float64 restatement of the library's ``step``.  Same
    relative bars as the DDIM and UniPC trajectories (test_e2e_gpu._traj_bar)."""
    from tests.test_e2e_gpu import _traj_bar
    p = small_pair
    steps, gs = 10, 7.0
    lat = g(42, 1, 4, 16, 16)
    vn = [g(400 + i, 1, 4, 16, 16) for i in range(steps)]
    ref = _oracle_run(p, name, lat, steps, gs, vn)
    out = _pipe(p, _mk(name))(**_call_kw(lat, steps, gs, **(dict(variance_noise=[v.cuda() for v in vn]) if name == "euler_a" else {}))).images
    st = err_stats(out, ref)
    print(f"pipeline_{name}_10_steps[{p['dtype']}]: {st}")
    bar = _traj_bar(p["dtype"])
    assert torch.isfinite(out).all()
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st


@pytest.mark.parametrize("name", ["dpm", "euler", "pndm"])
@torch.no_grad()
def test_step_graph_replay_of_the_samplers_is_bit_identical(small_pair, name):
    """enable_step_graph with three requests of different guidance: step 0 eager, one captured step replayed with a coefficient row
    per step (low-order start-up rows and the history slot included) == the eager loop, bit for bit, twice."""
    from tests.test_multi_request_gpu import _Requests
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _mk(name))
    pipe.enable_step_graph(False)
    eager = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
    pipe.enable_step_graph(True)
    try:
        g1 = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
        assert getattr(pipe, "_last_step_graph", None) is not None          # the graph path really ran
        g2 = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
    finally:
        pipe.enable_step_graph(False)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, g1) and torch.equal(eager, g2), (eager - g1).abs().max().item()


@torch.no_grad()
def test_euler_ancestral_runs_eagerly_under_step_graph(small_pair):
    pipe = _pipe(small_pair, _mk("euler_a"))
    lat = g(42, 1, 4, 16, 16)
    vn = [g(400 + i, 1, 4, 16, 16).cuda() for i in range(6)]
    a = pipe(**_call_kw(lat, 6, 7.0, variance_noise=vn)).images
    pipe.enable_step_graph(True)
    try:
        b = pipe(**_call_kw(lat, 6, 7.0, variance_noise=vn)).images
        assert getattr(pipe, "_last_step_graph", None) is None
    finally:
        pipe.enable_step_graph(False)
    assert torch.equal(a, b)
    c = pipe(**_call_kw(lat, 6, 7.0, generator=torch.Generator("cuda").manual_seed(5))).images
    d = pipe(**_call_kw(lat, 6, 7.0, generator=torch.Generator("cuda").manual_seed(5))).images
    e = pipe(**_call_kw(lat, 6, 7.0, generator=torch.Generator("cuda").manual_seed(6))).images
    assert torch.equal(c, d) and not torch.equal(c, e)
    with pytest.raises(ValueError, match="variance_noise"):
        pipe(**_call_kw(lat, 6, 7.0, variance_noise=vn[:3]))


@torch.no_grad()
def test_dpm_batched_guidance_matches_solo_calls(small_pair):
    """two requests with guidance 5.0 / 9.0 in one DPM-Solver++ call against two solo calls (the scalar step): the bars of
    test_batched_matches_solo_calls"""
    from tests.test_multi_request_gpu import _bar_small, _check, _Requests
    p, reqs = small_pair, _Requests(R=2)
    pipe = _pipe(p, _mk("dpm"))
    guidance = (5.0, 9.0)
    out = pipe(num_inference_steps=12, **reqs.call_kwargs(n=2, guidance=guidance)).images
    assert out.shape == (4, 4, 16, 16)
    for r in range(2):
        solo = pipe(num_inference_steps=12, **reqs.solo_kwargs(r, n=2, guidance=guidance)).images
        st = _check(out[2 * r:2 * r + 2], solo, _bar_small(p["dtype"]))
        print(f"dpm batched vs solo, request {r} [{p['dtype']}]: {st}")
    assert not torch.equal(out[:2], out[2:])


@pytest.mark.parametrize("name", ["euler", "dpm"])
@torch.no_grad()
def test_pipeline_inpaint_samplers_strength(name):
    """The inpainting pipeline at strength 0.6 with the scheduler's own add_noise coefficients in the start latents and in the
    per-step blend: the last step's blend target is noise-free, so outside the mask the result IS the image latent; inside it is
    finite.  And the whole trajectory matches the oracle loop (which blends with the restatement's add_noise)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    from oracle.pipeline import denoise
    from tests.test_e2e_gpu import _traj_bar
    dtype = torch.float16
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dtype)
    steps, gs, strength = 10, 5.0, 0.6
    noise = g(42, 1, 4, 16, 24)
    pe, ne = g(10, 1, 77, 64, scale=0.5), g(11, 1, 77, 64, scale=0.5)
    cloth = g(12, 2, 16, 64, scale=0.5); refl = g(13, 1, 4, 16, 16)
    img_lat = g(17, 1, 4, 16, 24)
    mask = torch.zeros(1, 1, 16, 24); mask[:, :, 4:12, 6:18] = 1.0
    ctrl = torch.rand(1, 3, 128, 192, generator=torch.Generator().manual_seed(18))
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_mk(name))
    mine = []
    out = pipe(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=192, height=128,
               num_inference_steps=steps, guidance_scale=gs, control_image=ctrl.cuda(), prompt_embeds=pe.cuda(),
               negative_prompt_embeds=ne.cuda(), ref_clip_hidden_states=cloth[1:2].cuda(), ref_image_latents=refl.cuda(),
               image_latents=img_lat.cuda(), mask_latents=mask.cuda(), noise=noise.cuda(), output_type="latent", strength=strength,
               trace=mine).images
    assert len(mine) == 6
    keep = (mask == 0).expand(1, 4, -1, -1)
    assert torch.allclose(out.cpu()[keep], img_lat[keep], atol=1e-5)
    assert torch.isfinite(out).all() and (out.cpu()[~keep] - img_lat[~keep]).abs().max() > 1e-2
    tr = []
    ref = denoise(p["o_unet"], p["o_ref"], ORACLES[name](), None, pe, ne, cloth, refl, steps, gs, controlnet=p["o_ctrl"],
                  control_image=ctrl, prompt_embeds_control=torch.cat([ne, pe]), conditioning_scale=1.0,
                  inpaint=dict(mask=mask, image_latents=img_lat, noise=noise), strength=strength, trace=tr)
    assert len(tr) == 6
    st = err_stats(out, ref)
    print(f"pipeline_inpaint_{name}_strength[{dtype}]: {st}")
    bar = _traj_bar(dtype)
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st
