"""Per-request ControlNet scale and guidance window in request-batched pipeline calls (``enable_request_control_scales``) on the GPU:
SMALL config, latent 16 x 16, 8 steps, the two-request ControlNet setting of tests/test_multi_request_gpu.py::test_controlnet_two_requests
(those requests, pose images and guidance values).

* parity: a mixed call against the reference loop at batch 1 driving the gated oracle ControlNet (tests/control_rows_oracle.py);
* isolation, bit for bit: what one request gets does not depend on the other request's scale;
* sensitivity: the scale and the window do change the result;
* equal values: the switch on with [0.8, 0.8] is the switch off with 0.8 -- the same bits and the same library calls;
* step graph: replay of the rows route, windows included, is bit-identical to the eager loop (DDIM, DPM-Solver++);
* composition (inpainting with strength 0.75, DeepCache (2, 1), two images per request, the IP-Adapter pipeline with faces): request 0
  of a rows-route call with the triple (0.5, 0, 0.5) against request 0 of the FOLDED call in which both requests have that triple.  The
  two differ by the extra rounding RNE16(s RNE16(y)) vs RNE16(s y) alone, which is exact in bf16 for a power of two (and for the closed
  gate, 0): bit-equal there -- a wrong step index, row order or uncond half could not be.  fp16 is exact too except where s y is
  subnormal, so it is held to the project's bar for the path (``_traj_bar``) against the folded result."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.control_rows_oracle import GatedControlNet  # noqa: E402
from tests.harness import SMALL, build_pair, err_stats  # noqa: E402
from tests.test_multi_request_gpu import _Requests, _check, _sched, _traj_bar, g  # noqa: E402

STEPS, GS = 8, (5.0, 7.0)
MIXED = dict(controlnet_conditioning_scale=[0.8, 0.4], control_guidance_start=[0.0, 0.25], control_guidance_end=[1.0, 0.75])
POW2 = dict(controlnet_conditioning_scale=[0.5, 0.25], control_guidance_start=[0.0, 0.0], control_guidance_end=[0.5, 1.0])          # rows route
POW2_FOLDED = dict(controlnet_conditioning_scale=[0.5, 0.5], control_guidance_start=[0.0, 0.0], control_guidance_end=[0.5, 0.5])     # request 0's triple, twice
_ORACLE = {}


def _pose():
    return [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r)) for r in range(2)]


def _dpm():
    from imagdressing_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _record(line):
    """every measured value: printed, and appended to the file IMD_CONTROL_ROWS_ACCURACY names (profiles/control_rows_accuracy.txt)"""
    print(line)
    path = os.environ.get("IMD_CONTROL_ROWS_ACCURACY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def setup(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    dt = request.param
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dt)
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    reqs = _Requests(R=2)
    cache = {}

    def call(on, n=1, steps=STEPS, **ctl):
        """one pipeline call of the two requests -> final latents [2 n, 4, 16, 16]; a result is computed once and never modified"""
        key = (on, n, steps, type(pipe.scheduler).__name__, bool(getattr(pipe, "_step_graph", False)), getattr(pipe, "_deepcache", None),
               tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in ctl.items())))
        if key not in cache:
            pipe.enable_request_control_scales(on)
            try:
                cache[key] = pipe(num_inference_steps=steps, pose_image=torch.cat(_pose()).cuda(),
                                  **reqs.call_kwargs(n=n, guidance=GS, image_scale=(1.0, 1.0)), **ctl).images.clone()
            finally:
                pipe.disable_request_control_scales()
        return cache[key]
    return dict(p=p, pipe=pipe, reqs=reqs, dtype=dt, call=call)


def _oracle(p, reqs, r, scale, start, end):
    key = (r, scale, start, end)
    if key not in _ORACLE:          # (the oracle is fp32 on the CPU: one run serves both element types)
        from oracle.ddim import DDIMOracle
        from oracle.pipeline import denoise
        gated = GatedControlNet(p["o_ctrl"], STEPS, start, end)
        _ORACLE[key] = denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r), reqs.pe[r], reqs.ne[r], reqs.cloth[r], reqs.refl[r], STEPS,
                               GS[r], controlnet=gated, control_image=_pose()[r], prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]),
                               conditioning_scale=scale)
        assert gated.calls == STEPS
    return _ORACLE[key]


@torch.no_grad()
def test_mixed_call_matches_each_requests_own_oracle_run(setup):
    """Bar: the project's ``_traj_bar``.  Should a request miss it, the yardstick is the parent's behaviour: the same request as a solo
    folded call against the same oracle run, which the mixed call may exceed by 10 % (one more 16-bit rounding of the residuals sits
    below the roundings already in that path; the margin covers batch-2 against batch-1 tile choices)."""
    p, reqs, dt, pipe = setup["p"], setup["reqs"], setup["dtype"], setup["pipe"]
    out = setup["call"](True, **MIXED)
    bar = _traj_bar(dt)
    for r in range(2):
        triple = tuple(MIXED[k][r] for k in MIXED)
        ref = _oracle(p, reqs, r, *triple)
        st = err_stats(out[r:r + 1], ref)
        _record(f"control_rows parity {dt} request {r} {triple}: mixed call max_abs {st['max_abs']:.4e} rel_rms {st['rel_rms']:.4e} "
                f"ref_std {st['ref_std']:.4f} (bar max_abs {bar['max_abs']} x max(ref_std, 1), rel_rms {bar['rel_rms']})")
        assert torch.isfinite(out).all()
        if st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"]:
            continue
        solo = pipe(num_inference_steps=STEPS, pose_image=_pose()[r].cuda(), controlnet_conditioning_scale=triple[0], control_guidance_start=triple[1],
                    control_guidance_end=triple[2], **reqs.solo_kwargs(r, guidance=GS, image_scale=(1.0, 1.0))).images
        ss = err_stats(solo, ref)
        _record(f"control_rows parity {dt} request {r}: solo folded call max_abs {ss['max_abs']:.4e} rel_rms {ss['rel_rms']:.4e}")
        assert st["max_abs"] <= 1.1 * ss["max_abs"] and st["rel_rms"] <= 1.1 * ss["rel_rms"], (st, ss)


@torch.no_grad()
def test_a_requests_bits_do_not_depend_on_the_other_requests_scale(setup):
    call = setup["call"]
    a, b = call(True, controlnet_conditioning_scale=[1.0, 0.5]), call(True, controlnet_conditioning_scale=[1.0, 1.0])          # rows / folded
    assert torch.equal(a[0], b[0])
    c, d = call(True, controlnet_conditioning_scale=[0.8, 0.5]), call(True, controlnet_conditioning_scale=[0.8, 0.3])          # rows / rows
    assert torch.equal(c[0], d[0])
    # sensitivity: the other request does change with its scale, and a window changes the result
    assert not torch.equal(a[1], b[1]) and not torch.equal(c[1], d[1])
    rel = ((a[1] - b[1]).pow(2).mean().sqrt() / b[1].pow(2).mean().sqrt()).item()
    w = call(True, controlnet_conditioning_scale=[1.0, 0.5], control_guidance_end=[0.5, 1.0])
    relw = ((w[0] - a[0]).pow(2).mean().sqrt() / a[0].pow(2).mean().sqrt()).item()
    _record(f"control_rows sensitivity {setup['dtype']}: request 1 at 0.5 against 1.0 rel rms {rel:.4e}; request 0 window (0, 0.5) against (0, 1) rel rms {relw:.4e}")
    assert rel > 1e-3 and relw > 1e-3
    assert torch.equal(w[1], a[1])                                           # ... and the window of request 0 leaves request 1's bits alone


@torch.no_grad()
def test_equal_values_are_the_switch_off_call_bits_and_library_calls(setup):
    from imagdressing_amd import _lib, ops
    from tools.guidance_rescale_bench import CountingLib
    pipe, reqs = setup["pipe"], setup["reqs"]
    kw = dict(num_inference_steps=STEPS, pose_image=torch.cat(_pose()).cuda(), **reqs.call_kwargs(guidance=GS, image_scale=(1.0, 1.0)))
    real, counts, outs = _lib.load(), {}, {}
    arms = {"off": (False, dict(controlnet_conditioning_scale=0.8)), "on equal": (True, dict(controlnet_conditioning_scale=[0.8, 0.8])),
            "on windows equal": (True, dict(controlnet_conditioning_scale=[0.8, 0.8], control_guidance_start=[0.0, 0.0], control_guidance_end=1.0)),
            "on mixed": (True, dict(MIXED))}
    launches = ops.SCALE_ROWS_COUNTER["launches"]
    for arm, (on, ctl) in arms.items():
        pipe.enable_request_control_scales(on)
        _lib._lib = proxy = CountingLib(real)
        try:
            outs[arm] = pipe(**kw, **ctl).images
        finally:
            _lib._lib = real
            pipe.disable_request_control_scales()
        counts[arm] = dict(proxy.counts)
        if arm != "on mixed":
            assert ops.SCALE_ROWS_COUNTER["launches"] == launches            # the folded route never launches the row scale
    assert torch.equal(outs["off"], outs["on equal"]) and torch.equal(outs["off"], outs["on windows equal"])
    assert counts["off"] == counts["on equal"] == counts["on windows equal"] and "imd_residual_scale_rows" not in counts["off"]
    extra = {k: v - counts["off"].get(k, 0) for k, v in counts["on mixed"].items() if v != counts["off"].get(k, 0)}
    assert extra == {"imd_residual_scale_rows": STEPS}, extra                # the rows route: that one launch per step, nothing else
    # switch off: the differing list still raises, naming the argument
    with pytest.raises(ValueError, match="controlnet_conditioning_scale is per call"):
        pipe(**kw, controlnet_conditioning_scale=[0.8, 0.4])


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp"])
@torch.no_grad()
def test_step_graph_replays_the_rows_route_bit_for_bit(setup, sampler):
    pipe, call = setup["pipe"], setup["call"]
    pipe.scheduler = _sched() if sampler == "ddim" else _dpm()
    try:
        eager = call(True, **MIXED)
        pipe.enable_step_graph(True)
        pipe._last_step_graph = None
        g1 = call(True, **MIXED)
        assert getattr(pipe, "_last_step_graph", None) is not None            # it did replay: the gate changes over the steps on this call
        assert torch.isfinite(eager).all() and torch.equal(eager, g1), (eager - g1).abs().max().item()
    finally:
        pipe.enable_step_graph(False)
        pipe.scheduler = _sched()


def _compare_request0(dt, rows, folded, what):
    """request 0 of the rows-route call against request 0 of the folded call of its triple (see the module docstring)"""
    assert torch.isfinite(rows).all() and rows.shape == folded.shape
    n = rows.shape[0] // 2
    if dt is torch.bfloat16:
        assert torch.equal(rows[:n], folded[:n]), (what, (rows[:n] - folded[:n]).abs().max().item())
    else:
        _check(rows[:n], folded[:n], _traj_bar(dt), floor=1.0)
    assert not torch.equal(rows[n:], folded[n:])                             # request 1 has another triple


@torch.no_grad()
def test_composes_with_two_images_per_request(setup):
    call = setup["call"]
    _compare_request0(setup["dtype"], call(True, n=2, **POW2), call(True, n=2, **POW2_FOLDED), "n = 2")
    assert not torch.equal(call(True, n=2, **POW2)[0], call(True, n=2, **POW2)[1])          # (two images: two latents)


@torch.no_grad()
def test_composes_with_deepcache(setup):
    pipe, call = setup["pipe"], setup["call"]
    pipe.enable_deepcache(cache_interval=2, depth=1)
    try:
        _compare_request0(setup["dtype"], call(True, **POW2), call(True, **POW2_FOLDED), "deepcache (2, 1)")
        cached = call(True, **POW2)
    finally:
        pipe.disable_deepcache()
    assert not torch.equal(cached, call(True, **POW2))                        # the cache was on


@torch.no_grad()
def test_composes_with_inpainting_at_strength(setup):
    """strength 0.75 of 8 steps: 6 steps run, the gate is over those (the pipeline's own rule for its scalar): (0, 0.5) closes after 3"""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    p, dt = setup["p"], setup["dtype"]
    pe, ne = [g(10 + r, 1, 77, 64, scale=0.5) for r in range(2)], [g(20 + r, 1, 77, 64, scale=0.5) for r in range(2)]
    cloth, refl = [g(30 + r, 2, 16, 64, scale=0.5) for r in range(2)], [g(40 + r, 1, 4, 16, 16) for r in range(2)]
    img_lat, noise = [g(50 + r, 1, 4, 16, 24) for r in range(2)], [g(60 + r, 1, 4, 16, 24) for r in range(2)]
    mask = [torch.zeros(1, 1, 16, 24) for _ in range(2)]
    mask[0][:, :, 4:12, 6:18] = 1.0
    mask[1][:, :, 2:14, 3:10] = 1.0
    ctrl = [torch.rand(1, 3, 128, 192, generator=torch.Generator().manual_seed(70 + r)) for r in range(2)]
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched()).enable_request_control_scales()

    def run(**ctl):
        return pipe(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=192, height=128, num_inference_steps=STEPS,
                    guidance_scale=list(GS), strength=0.75, control_image=torch.cat(ctrl).cuda(), prompt_embeds=torch.cat(pe).cuda(),
                    negative_prompt_embeds=torch.cat(ne).cuda(), ref_clip_hidden_states=torch.cat([c[1:2] for c in cloth]).cuda(),
                    ref_image_latents=torch.cat(refl).cuda(), image_latents=torch.cat(img_lat).cuda(), mask_latents=torch.cat(mask).cuda(),
                    noise=torch.cat(noise).cuda(), output_type="latent", **ctl).images
    rows, folded = run(**POW2), run(**POW2_FOLDED)
    _compare_request0(dt, rows, folded, "inpainting, strength 0.75")
    full = run(controlnet_conditioning_scale=[0.5, 0.25])                     # no window: the gate of request 0 stays open for all 6 steps
    assert not torch.equal(full[0], rows[0])
    for r in range(2):                                                       # the blend: each request keeps ITS person outside ITS mask
        keep = (mask[r] == 0).expand(1, 4, -1, -1)
        assert torch.allclose(rows[r:r + 1].cpu()[keep], img_lat[r][keep], atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_composes_with_the_ip_adapter_pipeline_and_faces(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_ipa_controlnet import IMAGDressing_v1
    p = build_pair(SMALL, seed=3, kind="ipa", with_controlnet=True, dtype=dtype)
    reqs = _Requests(R=2)
    face_p, face_n = [g(80 + r, 1, 4, 64, scale=0.5) for r in range(2)], [g(90 + r, 1, 4, 64, scale=0.5) for r in range(2)]

    class FaceProj:      # image_proj_model stand-in: the face clip hidden states carry the request index (+ r + 1 cond, -(r + 1) uncond)
        def __call__(self, idv, clip):
            idx = clip[:, 0, 0].round().long().tolist()
            return torch.cat([face_p[i - 1] if i > 0 else face_n[-i - 1] for i in idx]).cuda()
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, ip_ckpt=None, scheduler=_sched())
    pipe.image_proj_model = FaceProj()
    pipe.enable_request_control_scales()
    fc, fu = torch.zeros(2, 257, 1280), torch.zeros(2, 257, 1280)
    for r in range(2):
        fc[r, 0, 0], fu[r, 0, 0] = r + 1, -(r + 1)
    pose = _pose()

    def run(**ctl):
        return pipe(num_inference_steps=STEPS, pose_image=[pose[0].cuda(), pose[1].cuda()], faceid_embeds=torch.ones(2, 512),
                    face_clip_hidden_states=fc, face_uncond_clip_hidden_states=fu, ipa_scale=0.9, s_lora_scale=0.2, c_lora_scale=0.2,
                    **reqs.call_kwargs(guidance=(7.0, 5.5), image_scale=(1.0, 1.0)), **ctl).images
    _compare_request0(dtype, run(**POW2), run(**POW2_FOLDED), "IP-Adapter pipeline with faces")
