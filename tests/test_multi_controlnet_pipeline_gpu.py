"""Several ControlNets in pipeline calls on the GPU: SMALL config, latent 16 x 16, 8 steps, two nets from different seeds, the two
requests of tests/test_multi_request_gpu.py.

* parity: a two-net call against the reference loop on the fp32 oracle driving the SUM of two gated oracle ControlNets
  (tests/multi_controlnet_oracle.py), at the project's bar for the path (``_traj_bar``); the one-net call of the same run is recorded
  next to it;
* ``MultiControlNetModel([a])`` is ``a``: the same bits, the same library calls per entry point;
* a gated net contributes nothing: ``[a, b]`` at ``[0.5, 0]`` against ``a`` alone at 0.5 -- the difference is the extra rounding
  RNE16(s RNE16(y)) against RNE16(s y), exact in bf16 for a power of two (bit-equal), held to ``_traj_bar`` in fp16;
* plumbing: ``[a, b]`` against ``[b, a]`` with images and scales swapped is bit-identical (a two-term fp32 sum commutes), and an image
  or a scale attached to the wrong net is not;
* graph replay is the eager loop bit for bit with windows that close one net and open the other late, and the eager loop runs fewer
  ControlNet forwards than nets x steps;
* a request's bits do not depend on the other request's per-net values; the second net's scale changes the result;
* composition: the inpainting pipeline (built-in condition + a pose net, strength 0.75), the IP-Adapter pipeline with faces,
  DeepCache (2, 1), two images per request -- each by the gated-net and the swap properties above."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.control_rows_oracle import GatedControlNet  # noqa: E402
from tests.harness import SMALL, build_pair, err_stats  # noqa: E402
from tests.multi_controlnet_oracle import SummedControlNets, second_controlnet  # noqa: E402
from tests.test_multi_request_gpu import _Requests, _check, _sched, _traj_bar, g  # noqa: E402

STEPS, GS = 8, (5.0, 7.0)
SCALES = [0.8, 0.6]
WINDOW = dict(control_guidance_start=[0.25, 0.0], control_guidance_end=[1.0, 0.5])          # net 0 opens late, net 1 closes halfway
_ORACLE = {}


def _pose(net):
    """the control images of net ``net``, one per request"""
    return [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r + 40 * net)) for r in range(2)]


def _images(order=(0, 1)):
    return [torch.cat(_pose(k)).cuda() for k in order]


def _dpm():
    from imagdressing_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _record(line):
    """every measured value: printed, and appended to the file IMD_MULTI_CONTROLNET_ACCURACY names (profiles/multi_controlnet_accuracy.txt)"""
    print(line)
    path = os.environ.get("IMD_MULTI_CONTROLNET_ACCURACY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _key(v):
    return tuple(_key(x) for x in v) if isinstance(v, (list, tuple)) else v


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def setup(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    dt = request.param
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dt)
    o_b, e_b = second_controlnet(SMALL, 31, dt)
    nets, o_nets = [p["e_ctrl"], e_b], [p["o_ctrl"], o_b]
    reqs = _Requests(R=2)
    pipes, cache = {}, {}

    def pipe_of(order):
        """the pipeline on the nets ``order`` (a tuple of net indices -> controlnet=[...]; an int -> that net itself)"""
        if order not in pipes:
            cn = nets[order] if isinstance(order, int) else [nets[k] for k in order]
            pipes[order] = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                                           controlnet=cn, image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
        return pipes[order]

    def call(order=(0, 1), n=1, on=False, images=None, **ctl):
        """one pipeline call of the two requests -> final latents [2 n, 4, 16, 16]; a result is computed once and never modified"""
        pipe = pipe_of(order)
        key = (order, n, on, images, type(pipe.scheduler).__name__, bool(getattr(pipe, "_step_graph", False)), getattr(pipe, "_deepcache", None),
               tuple(sorted((k, _key(v)) for k, v in ctl.items())))
        if key not in cache:
            pose = torch.cat(_pose(order)).cuda() if isinstance(order, int) else _images(images or order)
            pipe.enable_request_control_scales(on)
            try:
                cache[key] = pipe(num_inference_steps=STEPS, pose_image=pose, **reqs.call_kwargs(n=n, guidance=GS, image_scale=(1.0, 1.0)),
                                  **ctl).images.clone()
            finally:
                pipe.disable_request_control_scales()
        return cache[key]
    return dict(p=p, nets=nets, o_nets=o_nets, reqs=reqs, dtype=dt, call=call, pipe_of=pipe_of)


def _oracle(setup, r, order, scales):
    """the oracle run of request r on the nets ``order`` (fp32 on the CPU: one run serves both element types)"""
    key = (r, order, tuple(scales))
    if key not in _ORACLE:
        from oracle.ddim import DDIMOracle
        from oracle.pipeline import denoise
        p, reqs = setup["p"], setup["reqs"]
        if len(order) == 1:
            cn, image = GatedControlNet(setup["o_nets"][order[0]], STEPS), _pose(order[0])[r]
        else:
            cn, image = SummedControlNets([setup["o_nets"][k] for k in order], [_pose(k)[r] for k in order], scales, STEPS), None
        _ORACLE[key] = denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r), reqs.pe[r], reqs.ne[r], reqs.cloth[r], reqs.refl[r], STEPS,
                               GS[r], controlnet=cn, control_image=image, prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]),
                               conditioning_scale=scales[0])
        assert cn.calls == STEPS
    return _ORACLE[key]


def _same_but_for_the_rounding(dt, multi, single, what):
    """a multi-net call whose other nets are gated against the one-net folded call (see the module docstring)"""
    assert torch.isfinite(multi).all() and multi.shape == single.shape
    if dt is torch.bfloat16:
        assert torch.equal(multi, single), (what, (multi - single).abs().max().item())
    else:
        _check(multi, single, _traj_bar(dt), floor=1.0)


@torch.no_grad()
def test_two_nets_match_the_oracle_sum(setup):
    """Bar: the project's ``_traj_bar`` for the ControlNet path, for the two-net call as for the one-net call."""
    dt, call = setup["dtype"], setup["call"]
    bar = _traj_bar(dt)
    two, one = call(controlnet_conditioning_scale=SCALES), call(0, controlnet_conditioning_scale=SCALES[0])
    assert torch.isfinite(two).all()
    stats = []
    for r in range(2):
        st = err_stats(two[r:r + 1], _oracle(setup, r, (0, 1), SCALES))
        _record(f"multi_controlnet parity {dt} request {r} two nets {SCALES}: max_abs {st['max_abs']:.4e} rel_rms {st['rel_rms']:.4e} "
                f"ref_std {st['ref_std']:.4f} (bar max_abs {bar['max_abs']} x max(ref_std, 1), rel_rms {bar['rel_rms']})")
        stats.append(st)
    s1 = err_stats(one[0:1], _oracle(setup, 0, (0,), SCALES[:1]))
    _record(f"multi_controlnet parity {dt} request 0 one net {SCALES[0]}: max_abs {s1['max_abs']:.4e} rel_rms {s1['rel_rms']:.4e} "
            f"ref_std {s1['ref_std']:.4f}")
    for st in stats:
        assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st


@torch.no_grad()
def test_a_wrapper_of_one_net_is_that_net_bits_and_library_calls(setup):
    from imagdressing_amd import _lib, ops
    from imagdressing_amd.unet import MultiControlNetModel
    from tools.guidance_rescale_bench import CountingLib
    reqs, nets = setup["reqs"], setup["nets"]
    plain, listed = setup["pipe_of"](0), setup["pipe_of"]((0,))
    assert plain.controlnet is nets[0] and isinstance(listed.controlnet, MultiControlNetModel) and listed.controlnet.nets == [nets[0]]
    kw = dict(num_inference_steps=STEPS, pose_image=torch.cat(_pose(0)).cuda(), **reqs.call_kwargs(guidance=GS, image_scale=(1.0, 1.0)))
    real = _lib.load()
    mixes = ops.MIX_ROWS_COUNTER["launches"]
    for on, ctl in ((False, dict(controlnet_conditioning_scale=0.8, control_guidance_end=0.75)),
                    (True, dict(controlnet_conditioning_scale=[0.8, 0.4], control_guidance_start=[0.0, 0.25]))):          # folded / rows route
        outs, counts = [], []
        for pipe in (plain, listed):
            pipe.enable_request_control_scales(on)
            _lib._lib = proxy = CountingLib(real)
            try:
                outs.append(pipe(**kw, **ctl).images)
            finally:
                _lib._lib = real
                pipe.disable_request_control_scales()
            counts.append(dict(proxy.counts))
        assert torch.equal(outs[0], outs[1]) and counts[0] == counts[1] and "imd_residual_mix_rows" not in counts[1]
    assert ops.MIX_ROWS_COUNTER["launches"] == mixes


@torch.no_grad()
def test_a_gated_net_contributes_nothing(setup):
    dt, call = setup["dtype"], setup["call"]
    _same_but_for_the_rounding(dt, call(controlnet_conditioning_scale=[0.5, 0.0]), call(0, controlnet_conditioning_scale=0.5), "[0.5, 0] vs a")
    _same_but_for_the_rounding(dt, call(controlnet_conditioning_scale=[0.0, 0.5]), call(1, controlnet_conditioning_scale=0.5), "[0, 0.5] vs b")
    assert not torch.equal(call(controlnet_conditioning_scale=[0.5, 0.0]), call(controlnet_conditioning_scale=[0.0, 0.5]))
    # ... and a window that never opens is a scale of 0 at every step
    shut = call(controlnet_conditioning_scale=[0.5, 0.7], control_guidance_start=[0.0, 0.95])
    assert torch.equal(shut, call(controlnet_conditioning_scale=[0.5, 0.0]))


@torch.no_grad()
def test_images_and_scales_reach_their_own_net(setup):
    call = setup["call"]
    ab = call((0, 1), controlnet_conditioning_scale=SCALES, **WINDOW)
    ba = call((1, 0), controlnet_conditioning_scale=SCALES[::-1], control_guidance_start=WINDOW["control_guidance_start"][::-1],
              control_guidance_end=WINDOW["control_guidance_end"][::-1])
    assert torch.isfinite(ab).all() and torch.equal(ab, ba)
    assert not torch.equal(ab, call((0, 1), images=(1, 0), controlnet_conditioning_scale=SCALES, **WINDOW))                  # images swapped
    assert not torch.equal(ab, call((0, 1), controlnet_conditioning_scale=SCALES[::-1], **WINDOW))                          # scales swapped
    assert not torch.equal(ab, call((0, 1), controlnet_conditioning_scale=SCALES, control_guidance_start=[0.0, 0.25],
                                    control_guidance_end=[0.5, 1.0]))                                                        # windows swapped


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp"])
@torch.no_grad()
def test_step_graph_replays_the_mix_route_bit_for_bit(setup, sampler):
    from imagdressing_amd import _lib
    from tools.guidance_rescale_bench import CountingLib
    pipe, call, nets = setup["pipe_of"]((0, 1)), setup["call"], setup["nets"]
    pipe.scheduler = _sched() if sampler == "ddim" else _dpm()
    forwards = [0, 0]
    originals = [n.forward_nhwc for n in nets]

    def counting(k):
        def fwd(*a, **kw):
            forwards[k] += 1
            return originals[k](*a, **kw)
        return fwd
    real = _lib.load()
    try:
        for k, n in enumerate(nets):
            n.forward_nhwc = counting(k)
        _lib._lib = proxy = CountingLib(real)
        try:
            eager = pipe(num_inference_steps=STEPS, pose_image=_images(), controlnet_conditioning_scale=SCALES,
                         **setup["reqs"].call_kwargs(guidance=GS, image_scale=(1.0, 1.0)), **WINDOW).images.clone()
        finally:
            _lib._lib = real
        # net 0 is closed for 2 of the 8 steps, net 1 for 4: the eager loop does not run them there
        assert forwards == [6, 4] and sum(forwards) < 2 * STEPS
        assert proxy.counts["imd_residual_mix_rows"] == STEPS                  # one mix launch per step all the same
        pipe.enable_step_graph(True)
        pipe._last_step_graph = None
        replay = pipe(num_inference_steps=STEPS, pose_image=_images(), controlnet_conditioning_scale=SCALES,
                      **setup["reqs"].call_kwargs(guidance=GS, image_scale=(1.0, 1.0)), **WINDOW).images
        assert getattr(pipe, "_last_step_graph", None) is not None            # it did replay: the gates change over the steps on this call
        assert torch.isfinite(eager).all() and torch.equal(eager, replay), (eager - replay).abs().max().item()
    finally:
        for n in nets:
            del n.forward_nhwc
        pipe.enable_step_graph(False)
        pipe.scheduler = _sched()


@torch.no_grad()
def test_a_requests_bits_do_not_depend_on_the_other_requests_values(setup):
    call = setup["call"]
    a = call(on=True, controlnet_conditioning_scale=[[0.8, 0.5], [0.6, 0.3]], control_guidance_end=[[1.0, 0.5], 1.0])
    b = call(on=True, controlnet_conditioning_scale=[[0.8, 0.9], [0.6, 0.0]], control_guidance_end=[[1.0, 1.0], 1.0])
    assert torch.isfinite(a).all() and torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    # a list per request without the switch is refused by name
    with pytest.raises(ValueError, match=r"controlnet_conditioning_scale\[0\] is a list"):
        call(controlnet_conditioning_scale=[[0.8, 0.5], 0.6])
    with pytest.raises(ValueError, match="controlnet_conditioning_scale has 3 entries for 2 ControlNets"):
        call(controlnet_conditioning_scale=[0.8, 0.5, 0.1])
    with pytest.raises(ValueError, match="pose_image has 1 entries for 2 ControlNets"):
        setup["pipe_of"]((0, 1))(num_inference_steps=STEPS, pose_image=torch.cat(_pose(0)).cuda()[:1],
                                 **setup["reqs"].call_kwargs(guidance=GS, image_scale=(1.0, 1.0)))


@torch.no_grad()
def test_the_second_nets_scale_changes_the_result(setup):
    call = setup["call"]
    a, b = call(controlnet_conditioning_scale=SCALES), call(controlnet_conditioning_scale=[SCALES[0], 0.3])
    rel = ((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()).item()
    _record(f"multi_controlnet sensitivity {setup['dtype']}: net 1 at 0.3 against {SCALES[1]} rel rms {rel:.4e}")
    assert rel > 1e-3


@torch.no_grad()
def test_composes_with_two_images_per_request(setup):
    dt, call = setup["dtype"], setup["call"]
    multi = call(n=2, controlnet_conditioning_scale=[0.5, 0.0])
    _same_but_for_the_rounding(dt, multi, call(0, n=2, controlnet_conditioning_scale=0.5), "n = 2")
    assert multi.shape[0] == 4 and not torch.equal(multi[0], multi[1])          # (two images: two latents)
    assert torch.equal(call(n=2, controlnet_conditioning_scale=SCALES), call((1, 0), n=2, controlnet_conditioning_scale=SCALES[::-1]))


@torch.no_grad()
def test_composes_with_deepcache(setup):
    dt, call = setup["dtype"], setup["call"]
    pipes = [setup["pipe_of"](o) for o in ((0, 1), (1, 0), 0)]
    for pp in pipes:
        pp.enable_deepcache(cache_interval=2, depth=1)
    try:
        _same_but_for_the_rounding(dt, call(controlnet_conditioning_scale=[0.5, 0.0]), call(0, controlnet_conditioning_scale=0.5), "deepcache (2, 1)")
        cached = call(controlnet_conditioning_scale=SCALES, **WINDOW)
        assert torch.equal(cached, call((1, 0), controlnet_conditioning_scale=SCALES[::-1],
                                        control_guidance_start=WINDOW["control_guidance_start"][::-1],
                                        control_guidance_end=WINDOW["control_guidance_end"][::-1]))
    finally:
        for pp in pipes:
            pp.disable_deepcache()
    assert torch.isfinite(cached).all() and not torch.equal(cached, call(controlnet_conditioning_scale=SCALES, **WINDOW))          # the cache was on


@torch.no_grad()
def test_composes_with_inpainting_and_the_built_in_condition(setup):
    """the inpainting net on the built-in condition (control_image entry None) + a pose net, strength 0.75: 6 of 8 steps run"""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    from tests.inpaint_cases import noise_image, rect_mask
    from PIL import Image
    p, dt, nets = setup["p"], setup["dtype"], setup["nets"]
    person, mask_img = Image.fromarray(noise_image(2, (128, 128))), Image.fromarray(rect_mask((128, 128), (30, 90, 40, 100)))
    pose = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(77)).cuda()
    img_lat, noise = g(50, 1, 4, 16, 16), g(60, 1, 4, 16, 16)
    mask = torch.zeros(1, 1, 16, 16)
    mask[:, :, 4:12, 5:13] = 1.0

    def run(cn, control_image, **ctl):
        pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                               controlnet=cn, image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
        return pipe(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=STEPS,
                    guidance_scale=GS[0], strength=0.75, image=person, mask_image=mask_img, control_image=control_image,
                    prompt_embeds=g(10, 1, 77, 64, scale=0.5).cuda(), negative_prompt_embeds=g(20, 1, 77, 64, scale=0.5).cuda(),
                    ref_clip_hidden_states=g(30, 1, 16, 64, scale=0.5).cuda(), ref_image_latents=g(40, 1, 4, 16, 16).cuda(),
                    image_latents=img_lat.cuda(), mask_latents=mask.cuda(), noise=noise.cuda(), output_type="latent", **ctl).images
    single = run(nets[0], None, controlnet_conditioning_scale=0.5)
    _same_but_for_the_rounding(dt, run(nets, [None, pose], controlnet_conditioning_scale=[0.5, 0.0]), single, "inpainting, pose net gated")
    both = run(nets, [None, pose], controlnet_conditioning_scale=[0.5, 0.25], control_guidance_end=[1.0, 0.5])
    swapped = run(nets[::-1], [pose, None], controlnet_conditioning_scale=[0.25, 0.5], control_guidance_end=[0.5, 1.0])
    assert torch.isfinite(both).all() and torch.equal(both, swapped) and not torch.equal(both, single)
    keep = (mask == 0).expand(1, 4, -1, -1)                                   # the blend: the person stays outside the mask
    assert torch.allclose(both.cpu()[keep], img_lat[keep], atol=1e-5)
    with pytest.raises(ValueError, match="control_image: 2 of the 2 entries are None"):
        run(nets, [None, None])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_composes_with_the_ip_adapter_pipeline_and_faces(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_ipa_controlnet import IMAGDressing_v1
    p = build_pair(SMALL, seed=3, kind="ipa", with_controlnet=True, dtype=dtype)
    nets = [p["e_ctrl"], second_controlnet(SMALL, 31, dtype)[1]]
    reqs = _Requests(R=2)
    face_p, face_n = [g(80 + r, 1, 4, 64, scale=0.5) for r in range(2)], [g(90 + r, 1, 4, 64, scale=0.5) for r in range(2)]

    class FaceProj:      # image_proj_model stand-in: the face clip hidden states carry the request index (+ r + 1 cond, -(r + 1) uncond)
        def __call__(self, idv, clip):
            idx = clip[:, 0, 0].round().long().tolist()
            return torch.cat([face_p[i - 1] if i > 0 else face_n[-i - 1] for i in idx]).cuda()
    fc, fu = torch.zeros(2, 257, 1280), torch.zeros(2, 257, 1280)
    for r in range(2):
        fc[r, 0, 0], fu[r, 0, 0] = r + 1, -(r + 1)

    def run(cn, pose, **ctl):
        pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                               controlnet=cn, image_encoder=None, ImgProj=lambda h: h, ip_ckpt=None, scheduler=_sched())
        pipe.image_proj_model = FaceProj()
        return pipe(num_inference_steps=STEPS, pose_image=pose, faceid_embeds=torch.ones(2, 512),
                    face_clip_hidden_states=fc, face_uncond_clip_hidden_states=fu, ipa_scale=0.9, s_lora_scale=0.2, c_lora_scale=0.2,
                    **reqs.call_kwargs(guidance=(7.0, 5.5), image_scale=(1.0, 1.0)), **ctl).images
    per_request = [[_pose(k)[0].cuda(), _pose(k)[1].cuda()] for k in range(2)]          # a list per request inside each net's entry
    single = run(nets[0], per_request[0], controlnet_conditioning_scale=0.5)
    _same_but_for_the_rounding(dtype, run(nets, per_request, controlnet_conditioning_scale=[0.5, 0.0]), single, "IP-Adapter, net 1 gated")
    both = run(nets, per_request, controlnet_conditioning_scale=SCALES, **WINDOW)
    swapped = run(nets[::-1], per_request[::-1], controlnet_conditioning_scale=SCALES[::-1],
                  control_guidance_start=WINDOW["control_guidance_start"][::-1], control_guidance_end=WINDOW["control_guidance_end"][::-1])
    assert torch.isfinite(both).all() and torch.equal(both, swapped) and not torch.equal(both, single)
