"""In-flight batching on the GPU (``pipe.open_session`` / ``session.DenoiseSession``): requests that enter a running batch at different
steps and run different numbers of steps, against the reference loop at batch 1 with each request's own settings; isolation of a
request from its batch company; lockstep against the request-batched call; the ControlNet pipeline; the life cycle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair  # noqa: E402
from tests.test_multi_request_gpu import (R3_GUIDANCE, R3_IMAGE_SCALE, _bar_small, _check, _Requests, _sched,  # noqa: E402
                                          _set_oracle_image_scale, _traj_bar)

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _engine_scheduler(name):
    from imagdressing_amd import scheduler as S
    return {"ddim": _sched, "dpm": lambda: S.DPMSolverMultistepScheduler(**KW), "euler": lambda: S.EulerDiscreteScheduler(**KW),
            "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW)}[name]()


def _oracle_scheduler(name):
    from oracle.ddim import DDIMOracle
    from tests.sampler_oracle import DPMSolverOracle, EulerOracle
    return {"ddim": DDIMOracle, "dpm": DPMSolverOracle, "euler": EulerOracle}[name]()


_REF = {}


def _reference(p, reqs, name, r, steps):
    """oracle.pipeline.denoise at batch 1 with request r's own garment, prompt, guidance, image scale and step count (the fp32 CPU
    oracle is the same for both element types: computed once)"""
    key = (name, r, steps)
    if key not in _REF:
        from oracle.pipeline import denoise
        orc = _oracle_scheduler(name)
        orc.set_timesteps(steps)
        _set_oracle_image_scale(p["o_unet"], R3_IMAGE_SCALE[r])
        try:
            _REF[key] = denoise(p["o_unet"], p["o_ref"], orc, reqs.latent(r) * orc.init_noise_sigma, reqs.pe[r], reqs.ne[r], reqs.cloth[r],
                                reqs.refl[r], steps, R3_GUIDANCE[r])
        finally:
            _set_oracle_image_scale(p["o_unet"], 1.0)
    return _REF[key]


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


def _submit_kw(reqs, r, steps, guidance=R3_GUIDANCE, image_scale=R3_IMAGE_SCALE, **over):
    kw = dict(num_inference_steps=steps, guidance_scale=guidance[r], image_scale=image_scale[r], prompt_embeds=reqs.pe[r].cuda(),
              negative_prompt_embeds=reqs.ne[r].cuda(), ref_clip_hidden_states=reqs.cloth[r][1:2].cuda(), ref_image_latents=reqs.refl[r].cuda(),
              latents=reqs.latent(r).cuda(), output_type="latent")
    kw.update(over)
    return kw


@pytest.mark.parametrize("name", ["ddim", "dpm", "euler"])
@torch.no_grad()
def test_staggered_requests_match_the_reference_loop(small_pair, name):
    """2 slots, three distinct requests of 12, 8 and 10 steps: the first submitted before step 0, the second after step 3, the third
    right behind it -- queued, it inherits a used slot (stale latent, stale history).  Every final latent against the reference loop
    at batch 1 with that request's own settings: DDIM within the bars of the request-batched call, DPM-Solver++ and Euler within the
    trajectory bars those samplers have through the pipeline."""
    p, reqs = small_pair, _Requests()
    steps = (12, 8, 10)
    pipe = _pipe(p, _engine_scheduler(name))
    with pipe.open_session(slots=2, width=128, height=128) as ses:
        a = ses.submit(**_submit_kw(reqs, 0, steps[0]))
        assert a.slot is None and not a.done and a.steps_done == 0
        done = []
        for _ in range(4):
            done += ses.step()
        assert a.slot == 0 and a.steps_done == 4 and ses.free_slots == [1]
        b = ses.submit(**_submit_kw(reqs, 1, steps[1]))
        c = ses.submit(**_submit_kw(reqs, 2, steps[2]))
        done += ses.step()
        assert b.slot == 1 and c.slot is None and b.steps_done == 1 and a.steps_done == 5
        done += ses.drain()
        assert done == [a, b, c]
        assert c.slot == 0 and ses.steps_run == 12 + 10 and ses.free_slots == [0, 1]
        outs = [t.result().images for t in (a, b, c)]
    for r in range(3):
        assert outs[r].shape == (1, 4, 16, 16)
        ref = _reference(p, reqs, name, r, steps[r])
        if name == "ddim":
            st = _check(outs[r], ref, _bar_small(p["dtype"]))
        else:
            st = _check(outs[r], ref, _traj_bar(p["dtype"]), floor=1.0)
        print(f"session {name} request {r} ({steps[r]} steps) [{p['dtype']}]: {st}")


@pytest.mark.parametrize("name", ["dpm", "ddim"])
@torch.no_grad()
def test_a_request_does_not_see_its_batch_company(small_pair, name):
    """Request A in slot 0 of a 3-slot session: the same final latent, bit for bit, whether slots 1 and 2 stay idle or are taken by
    other requests at steps 2 and 5 -- every launch on the path is row-local."""
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _engine_scheduler(name))
    with pipe.open_session(slots=3, width=128, height=128) as ses:
        a = ses.submit(**_submit_kw(reqs, 0, 10))
        ses.drain()
        alone = a.result().images
    with pipe.open_session(slots=3, width=128, height=128) as ses:
        a = ses.submit(**_submit_kw(reqs, 0, 10))
        ses.step(), ses.step()
        b = ses.submit(**_submit_kw(reqs, 1, 12))
        ses.step(), ses.step(), ses.step()
        c = ses.submit(**_submit_kw(reqs, 2, 4))
        ses.drain()
        assert (a.slot, b.slot, c.slot) == (0, 1, 2) and ses.steps_run == 14
        crowded = a.result().images
        assert torch.isfinite(b.result().images).all() and torch.isfinite(c.result().images).all()
    assert torch.isfinite(alone).all()
    assert torch.equal(alone, crowded), (alone - crowded).abs().max().item()


@torch.no_grad()
def test_lockstep_matches_the_request_batched_call(small_pair):
    """three requests admitted together with equal step counts == the request-batched pipe(...) call, within the bars of that call
    (not bit for bit: the session's DDIM step is the affine row, the call's is imd_ddim_cfg_step)"""
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _sched())
    batched = pipe(num_inference_steps=8, **reqs.call_kwargs()).images
    with pipe.open_session(slots=3, width=128, height=128) as ses:
        tickets = [ses.submit(**_submit_kw(reqs, r, 8)) for r in range(3)]
        assert ses.drain() == tickets and ses.steps_run == 8
    for r in range(3):
        st = _check(tickets[r].result().images, batched[r:r + 1], _bar_small(p["dtype"]))
        print(f"session lockstep vs batched call, request {r} [{p['dtype']}]: {st}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_controlnet_session_staggered(dtype):
    """the ControlNet (pose) pipeline: two staggered requests with their own pose images against the oracle with its ControlNet.
    Both run 8 steps, the trajectory ``_traj_bar`` was set on (test_controlnet_two_requests: these requests, guidance and
    conditioning scale): the bar carries no meaning at another step count.  Measured: with 6 steps a bf16 SOLO pipeline call of request 1
    -- no session involved -- lands at rel_rms 2.78e-2 (the session at the same 2.78e-2, 8 steps: both 2.46e-2; fp16 3.2e-3 everywhere),
    and the session's rows equalled the session-alone rows bit for bit in every case."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dtype)
    reqs, steps, gs = _Requests(R=2), (8, 8), (5.0, 7.0)
    pose = [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r)) for r in range(2)]
    refs = [denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r), reqs.pe[r], reqs.ne[r], reqs.cloth[r], reqs.refl[r],
                    steps[r], gs[r], controlnet=p["o_ctrl"], control_image=pose[r], prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]),
                    conditioning_scale=0.8) for r in range(2)]
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    with pipe.open_session(slots=2, width=128, height=128, controlnet_conditioning_scale=0.8) as ses:
        with pytest.raises(ValueError, match="pose_image"):
            ses.submit(**_submit_kw(reqs, 0, steps[0], guidance=gs, image_scale=(1.0, 1.0)))
        with pytest.raises(NotImplementedError, match="control_guidance"):
            ses.submit(**_submit_kw(reqs, 0, steps[0], guidance=gs, image_scale=(1.0, 1.0), pose_image=pose[0].cuda(), control_guidance_end=0.5))
        a = ses.submit(**_submit_kw(reqs, 0, steps[0], guidance=gs, image_scale=(1.0, 1.0), pose_image=pose[0].cuda()))
        ses.step(), ses.step()
        b = ses.submit(**_submit_kw(reqs, 1, steps[1], guidance=gs, image_scale=(1.0, 1.0), pose_image=pose[1].cuda()))
        ses.drain()
        assert (a.slot, b.slot) == (0, 1) and ses.steps_run == 10
    for r, t in enumerate((a, b)):
        st = _check(t.result().images, refs[r], _traj_bar(dtype), floor=1.0)
        print(f"controlnet session request {r} [{dtype}]: {st}")


@torch.no_grad()
def test_session_life_cycle(small_pair):
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _engine_scheduler("dpm"))
    call = dict(num_inference_steps=6, **reqs.solo_kwargs(0))
    before = pipe(**call).images
    unet = p["e_unet"]
    ses = pipe.open_session(slots=2, width=128, height=128)
    assert ses.step() == [] and ses.steps_run == 0                       # nothing submitted: nothing launched
    # refusals name the option and leave the session usable
    with pytest.raises(NotImplementedError, match="guidance_scale <= 1"):
        ses.submit(**_submit_kw(reqs, 0, 6, guidance=(1.0, 1.0, 1.0)))
    with pytest.raises(ValueError, match="one geometry per session"):
        ses.submit(**_submit_kw(reqs, 0, 6, latents=torch.zeros(1, 4, 16, 24).cuda()))
    with pytest.raises(ValueError, match="width x height"):
        ses.submit(**_submit_kw(reqs, 0, 6, width=192))
    with pytest.raises(NotImplementedError, match="eta > 0"):
        ses.submit(**_submit_kw(reqs, 0, 6, eta=0.3))
    pipe.enable_deepcache(2)
    try:
        with pytest.raises(NotImplementedError, match="enable_deepcache"):
            ses.step()
    finally:
        pipe.disable_deepcache()
    pipe.enable_step_graph(True)                                          # ignored inside a session
    try:
        two = ses.submit(**_submit_kw(reqs, 1, 5, latents=torch.cat([reqs.latent(1, 0), reqs.latent(1, 1)]).cuda(), num_images_per_prompt=2))
        one = ses.submit(**_submit_kw(reqs, 0, 3))
        with pytest.raises(RuntimeError, match="has not finished"):
            two.result()
        assert ses.step() == [] and two.slots == [0, 1] and one.slot is None and two.steps_done == 1
        with pytest.raises(RuntimeError, match="has not finished"):
            two.result()
        assert ses.drain() == [two, one] and ses.free_slots == [0, 1] and ses.steps_run == 8
        assert getattr(pipe, "_last_step_graph", None) is None
    finally:
        pipe.enable_step_graph(False)
    out = two.result()
    assert out.images.shape == (2, 4, 16, 16) and torch.equal(out.images, two.latents) and not torch.equal(out.images[0], out.images[1])
    assert one.done and one.slot == 0 and one.steps_done == 3 and one.result().images.shape == (1, 4, 16, 16)
    # a step that raises: the encoders' time-embedding state does not leak out of it, and close() clears it whatever happened
    t = ses.submit(**_submit_kw(reqs, 2, 4))
    real = unet.forward_nhwc

    def boom(*a, **k):
        assert unet.__dict__.get("_temb_fixed") is not None              # (the per-row buffer is installed during the forward)
        raise RuntimeError("boom")
    unet.forward_nhwc = boom
    try:
        with pytest.raises(RuntimeError, match="boom"):
            ses.step()
    finally:
        unet.forward_nhwc = real
    assert unet.__dict__.get("_temb_fixed") is None and unet.__dict__.get("_temb_table") is None
    unet._temb_fixed = torch.zeros(1)                                     # whatever state a failure may have left behind
    ses.close()
    assert unet.__dict__.get("_temb_fixed") is None and ses.closed and ses.z is None
    with pytest.raises(RuntimeError, match="closed"):
        ses.step()
    with pytest.raises(RuntimeError, match="dropped"):
        t.result()
    ses.close()                                                           # idempotent
    after = pipe(**call).images
    assert torch.equal(before, after)
