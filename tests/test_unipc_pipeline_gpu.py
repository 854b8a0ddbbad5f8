"""UniPC with the fused-step switch on, through the pipelines and the sessions (SMALL config, 16 x 16 latents, 10 steps): against the
reference loop driven by oracle/unipc.py, the switch-off route driven by hand, graph replay, request batches with their own guidance
scales, the inpainting pipeline at strength 1 and 0.6, DeepCache, and denoising sessions with and without compaction."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair, err_stats  # noqa: E402
from tests.test_e2e_gpu import _traj_bar  # noqa: E402
from tests.test_multi_request_gpu import R3_GUIDANCE, _Requests  # noqa: E402
from tests.unipc_cases import KW, StartOracle  # noqa: E402

STEPS, GS = 10, 7.0


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


PE, NE = g(10, 1, 77, 64, scale=0.5), g(11, 1, 77, 64, scale=0.5)
CLOTH, REFL = g(12, 2, 16, 64, scale=0.5), g(13, 1, 4, 16, 16)
LAT = g(42, 1, 4, 16, 16)


def _sched(on=True, **kw):
    from imagdressing_amd.scheduler import UniPCMultistepScheduler
    return UniPCMultistepScheduler(fused_step=on, **kw, **KW)


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def pair(request):
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=request.param)
    p["dtype"] = request.param
    return p


def _pipe(p, sch):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    return IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           image_encoder=None, ImgProj=lambda h: h, scheduler=sch, safety_checker=None, feature_extractor=None)


def _kw(lat=LAT, steps=STEPS, gs=GS, **over):
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=steps,
              guidance_scale=gs, num_images_per_prompt=lat.shape[0], prompt_embeds=PE.cuda(), negative_prompt_embeds=NE.cuda(),
              ref_clip_hidden_states=CLOTH[1:2].cuda(), ref_image_latents=REFL.cuda(), latents=lat.cuda(), output_type="latent")
    kw.update(over)
    return kw


def _check(out, ref, dtype, what):
    st = err_stats(out, ref)
    print(f"{what}[{dtype}]: {st}")
    bar = _traj_bar(dtype)
    assert torch.isfinite(out).all()
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st
    return st


_ORACLE = {}          # the fp32 CPU oracle is the same for both element types: every reference is computed once


def _oracle(key, make):
    if key not in _ORACLE:
        _ORACLE[key] = make()
    return _ORACLE[key]


# ---- the base pipeline ----
@torch.no_grad()
def test_switch_on_10_steps_vs_oracle(pair):
    """two images through the base pipeline against oracle.pipeline.denoise driven by UniPCOracle"""
    from oracle.pipeline import denoise
    from oracle.unipc import UniPCOracle
    p = pair
    lat = torch.stack([g(42 + i, 4, 16, 16) for i in range(2)])
    ref = _oracle("base", lambda: torch.cat([denoise(p["o_unet"], p["o_ref"], UniPCOracle(), lat[i:i + 1], PE, NE, CLOTH, REFL, STEPS, GS)
                                             for i in range(2)]))
    sch = _sched()
    trace = []
    out = _pipe(p, sch)(trace=trace, **_kw(lat)).images
    assert len(trace) == STEPS and sch.step_index == 0 and sch.model_outputs == []          # the three-launch state machine never ran
    _check(out, ref, p["dtype"], "pipeline_unipc_fused_10_steps")
    # order 3, bh1: the other coefficient families through the same launch
    ref3 = _oracle("base3", lambda: denoise(p["o_unet"], p["o_ref"], UniPCOracle(solver_order=3, solver_type="bh1"), LAT, PE, NE, CLOTH, REFL,
                                            STEPS, GS))
    _check(_pipe(p, _sched(solver_order=3, solver_type="bh1"))(**_kw()).images, ref3, p["dtype"], "pipeline_unipc_fused_order3_bh1")


@torch.no_grad()
def test_switch_off_is_the_three_launch_route(pair):
    """switch off: the pipeline's latents, bit for bit, are those of the parent's route driven by hand -- UNet, ``step_guided`` (three
    imd_lincomb launches), the identity imd_ddim_cfg_step that emits the UNet input -- and the refusals stand; switch on differs from
    it only at rounding level"""
    from imagdressing_amd import ops
    p, dt = pair, pair["dtype"]
    lat = torch.stack([g(42 + i, 4, 16, 16) for i in range(2)])
    sch = _sched(on=False)
    pipe = _pipe(p, sch)
    off = pipe(**_kw(lat)).images
    with pytest.raises(ValueError, match="UniPC"):
        pipe(**dict(_Requests().call_kwargs(), num_inference_steps=4))
    with pytest.raises(NotImplementedError, match="UniPC"):
        pipe.open_session(slots=2, width=128, height=128)
    # by hand
    B, HW = 2, 256
    hand = _sched(on=False)
    hand.set_timesteps(STEPS)
    ts = [int(t) for t in hand.timesteps]
    sa = pipe._sa_states(REFL.cuda(), CLOTH[1:2].cuda(), False, 1)
    ehs = torch.cat([PE, NE]).to(device="cuda", dtype=dt).contiguous()
    cak = {"sa_hidden_states": sa, "sa_batch_mask": torch.cat([torch.ones(B), torch.zeros(B)]).cuda(), "sa_pair_layout": True}
    z = lat.cuda().float().permute(0, 2, 3, 1).reshape(B, HW, 4).contiguous()
    x_in = torch.zeros(2 * B, 16, 16, 8, dtype=dt, device="cuda")
    x_in[..., :4] = torch.cat([z, z]).view(2 * B, 16, 16, 4)
    unet = p["e_unet"]
    unet.precompute_time_embeddings(ts, torch.device("cuda"))
    try:
        for t in ts:
            eps = unet.forward_nhwc(x_in, t, ehs, cak, None, None, cfg_pair=True)
            z = hand.step_guided(eps.view(2 * B, HW, 4), z, GS)
            ops.ddim_cfg_step(z, torch.zeros(2 * B, HW, 4, device="cuda"), x_in.view(2 * B, HW, 8), guidance=1.0, a_t=1.0, a_prev=1.0)
    finally:
        unet.clear_time_embeddings()
    want = z.view(B, 16, 16, 4).permute(0, 3, 1, 2)
    assert torch.isfinite(off).all() and torch.equal(off, want), (off - want).abs().max().item()
    on = _pipe(p, _sched())(**_kw(lat)).images
    st = err_stats(on, off)
    print(f"unipc switch on vs off [{dt}]: {st}")
    bar = _traj_bar(dt)
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st


@torch.no_grad()
def test_step_graph_replay_is_bit_identical(pair):
    """three requests of different guidance: step 0 eager, one captured step replayed with 19 coefficients per step from device memory
    == the eager loop, bit for bit, twice; with the switch off the graph is ignored as before"""
    p, reqs = pair, _Requests()
    pipe = _pipe(p, _sched())
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
    off = _pipe(p, _sched(on=False)).enable_step_graph(True)
    try:
        off(**_kw(steps=4))
        assert getattr(off, "_last_step_graph", None) is None
    finally:
        off.enable_step_graph(False)


@torch.no_grad()
def test_request_batch_with_three_guidance_scales(pair):
    """guidance 5.0 / 7.5 / 9.0 in one call == three solo calls within the trajectory bar; the same scale for all requests is
    bit-identical to the scalar-guidance call (the uniform case takes the scalar step)"""
    p, reqs = pair, _Requests()
    pipe = _pipe(p, _sched())
    out = pipe(num_inference_steps=STEPS, **reqs.call_kwargs()).images
    assert out.shape == (3, 4, 16, 16)
    for r in range(3):
        solo = pipe(num_inference_steps=STEPS, **reqs.solo_kwargs(r)).images
        _check(out[r:r + 1], solo, p["dtype"], f"unipc fused batched vs solo, request {r}")
    assert not torch.equal(out[0], out[1])
    same = pipe(num_inference_steps=STEPS, **reqs.call_kwargs(guidance=(7.5, 7.5, 7.5))).images
    scalar = pipe(num_inference_steps=STEPS, **dict(reqs.call_kwargs(), guidance_scale=7.5)).images
    assert torch.equal(same, scalar)


# ---- the inpainting pipeline ----
@pytest.mark.parametrize("strength", [1.0, 0.6])
@torch.no_grad()
def test_inpainting_pipeline(pair, strength):
    """``inpaint=`` and ``strength`` < 1 against the oracle loop with the blend applied between UniPCOracle steps (its last_sample
    stays unblended); outside the mask the final latent IS the image latent, exactly"""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    from oracle.pipeline import denoise
    p = pair
    gs = 5.0
    noise, img_lat = g(42, 1, 4, 16, 24), g(17, 1, 4, 16, 24)
    mask = torch.zeros(1, 1, 16, 24)
    mask[:, :, 4:12, 6:18] = 1.0
    ctrl = torch.rand(1, 3, 128, 192, generator=torch.Generator().manual_seed(18))
    run = min(int(STEPS * strength), STEPS)
    tr = []
    ref = _oracle(("inpaint", strength), lambda: denoise(
        p["o_unet"], p["o_ref"], StartOracle(start=STEPS - run), noise if strength == 1.0 else None, PE, NE, CLOTH, REFL, STEPS, gs,
        controlnet=p["o_ctrl"], control_image=ctrl, prompt_embeds_control=torch.cat([NE, PE]), conditioning_scale=1.0,
        inpaint=dict(mask=mask, image_latents=img_lat, noise=noise), strength=strength, trace=tr))
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    mine = []
    out = pipe(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=192, height=128,
               num_inference_steps=STEPS, guidance_scale=gs, control_image=ctrl.cuda(), prompt_embeds=PE.cuda(),
               negative_prompt_embeds=NE.cuda(), ref_clip_hidden_states=CLOTH[1:2].cuda(), ref_image_latents=REFL.cuda(),
               image_latents=img_lat.cuda(), mask_latents=mask.cuda(), noise=noise.cuda(), output_type="latent", strength=strength,
               trace=mine).images
    assert len(mine) == run
    keep = (mask == 0).expand(1, 4, -1, -1)
    assert torch.equal(out.cpu()[keep], img_lat[keep])                          # b_img = 1, b_noise = 0 after the last step
    assert (out.cpu()[~keep] - img_lat[~keep]).abs().max() > 1e-2
    _check(out, ref, p["dtype"], f"pipeline_inpaint_unipc_fused_strength_{strength}")


# ---- DeepCache ----
@torch.no_grad()
def test_deepcache(pair):
    """(3, 1): the full / shallow plan of the UNet calls is DPM-Solver++'s, and the trajectory follows the oracle loop on the cached
    oracle UNet; cache_interval = 1 is the loop without the cache, bit for bit"""
    from imagdressing_amd.dressing_sd.pipelines._base import deepcache_plan
    from imagdressing_amd.scheduler import DPMSolverMultistepScheduler
    from oracle.pipeline import denoise
    from oracle.unipc import UniPCOracle
    from tests.deepcache_oracle import DeepCacheUNet
    p = pair
    unet = p["e_unet"]
    real = unet.forward_nhwc

    def plan_of(pipe):
        seen = []

        def spy(*a, **k):
            seen.append(k["deepcache"].full if "deepcache" in k else None)
            return real(*a, **k)
        unet.forward_nhwc = spy
        try:
            out = pipe(**_kw()).images
        finally:
            unet.forward_nhwc = real
        return seen, out
    pipe = _pipe(p, _sched())
    plain = pipe(**_kw()).images
    pipe.enable_deepcache(cache_interval=1)
    assert torch.equal(pipe(**_kw()).images, plain)
    pipe.enable_deepcache(cache_interval=3, depth=1)
    mine, out = plan_of(pipe)
    pipe.disable_deepcache()
    theirs, _ = plan_of(_pipe(p, DPMSolverMultistepScheduler(**KW)).enable_deepcache(cache_interval=3, depth=1))
    assert mine == theirs == list(deepcache_plan(STEPS, 3)) and not all(mine)
    assert torch.equal(pipe(**_kw()).images, plain)

    def cached():
        orc = UniPCOracle()
        orc.set_timesteps(STEPS)
        return denoise(DeepCacheUNet(p["o_unet"], 3, 1, n_calls=STEPS + 1), p["o_ref"], orc, LAT, PE, NE, CLOTH, REFL, STEPS, GS)
    _check(out, _oracle("deepcache", cached), p["dtype"], "deepcache_unipc_fused_3_1")
    assert not torch.equal(out, plain)


# ---- sessions ----
def _submit_kw(reqs, r, steps):
    return dict(num_inference_steps=steps, guidance_scale=R3_GUIDANCE[r], image_scale=1.0, prompt_embeds=reqs.pe[r].cuda(),
                negative_prompt_embeds=reqs.ne[r].cuda(), ref_clip_hidden_states=reqs.cloth[r][1:2].cuda(), ref_image_latents=reqs.refl[r].cuda(),
                latents=reqs.latent(r).cuda(), output_type="latent")


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
@torch.no_grad()
def test_session(pair, compact):
    """base pipeline, 3 slots.  Request A's latents are bit-identical alone, beside idle slots, and beside requests admitted two steps
    later with other step counts (compacting: at the same widths, so the ladder is pinned to (3,)); every request equals its solo
    switch-on pipeline call within the trajectory bar -- bit for bit where width and tile choices coincide: the non-compacting
    session against the call at the same batch"""
    p, reqs = pair, _Requests()
    pipe = _pipe(p, _sched())
    kw = dict(slots=3, width=128, height=128, compact=compact, **(dict(widths=(3,)) if compact else {}))
    with pipe.open_session(**kw) as ses:
        a = ses.submit(**_submit_kw(reqs, 0, 10))
        ses.drain()
        alone = a.result().images
        assert ses.hist.shape[0] == 3 and ses.coef_rows.shape[1] == 24
    with pipe.open_session(**kw) as ses:
        a = ses.submit(**_submit_kw(reqs, 0, 10))
        ses.step(), ses.step()
        b = ses.submit(**_submit_kw(reqs, 1, 12))
        c = ses.submit(**_submit_kw(reqs, 2, 4))
        ses.drain()
        assert (a.slot, b.slot, c.slot) == (0, 1, 2) and ses.steps_run == 14
        crowded, others = a.result().images, (b.result().images, c.result().images)
    assert torch.isfinite(alone).all() and torch.equal(alone, crowded), (alone - crowded).abs().max().item()
    for r, (out, steps) in enumerate(((crowded, 10), (others[0], 12), (others[1], 4))):
        solo = pipe(**dict(reqs.solo_kwargs(r), num_inference_steps=steps, image_scale=1.0)).images
        _check(out, solo, p["dtype"], f"unipc fused session ({'compact' if compact else 'slots'}) request {r} vs its solo call")
    if compact:
        # the real ladder: widths 1, 2, 3 as requests come and go; still every request within the bar of its solo call
        with pipe.open_session(slots=3, width=128, height=128, compact=True) as ses:
            a = ses.submit(**_submit_kw(reqs, 0, 10))
            ses.step(), ses.step()
            b = ses.submit(**_submit_kw(reqs, 1, 12))
            c = ses.submit(**_submit_kw(reqs, 2, 4))
            ses.drain()
            assert set(ses.steps_at_width) == {1, 2, 3} and ses.repacks >= 2
            for r, (t, steps) in enumerate(((a, 10), (b, 12), (c, 4))):
                solo = pipe(**dict(reqs.solo_kwargs(r), num_inference_steps=steps, image_scale=1.0)).images
                _check(t.result().images, solo, p["dtype"], f"unipc fused session (ladder) request {r} vs its solo call")
    else:
        # the same batch, the same widths and tiles: three requests in lockstep == the request-batched call, bit for bit
        batched = pipe(num_inference_steps=8, **reqs.call_kwargs(image_scale=(1.0, 1.0, 1.0))).images
        with pipe.open_session(**kw) as ses:
            tickets = [ses.submit(**_submit_kw(reqs, r, 8)) for r in range(3)]
            assert ses.drain() == tickets and ses.steps_run == 8
        assert torch.equal(torch.cat([t.result().images for t in tickets]), batched)
