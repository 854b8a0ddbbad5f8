"""DeepCache on the GPU (``enable_deepcache``, ``unet.DeepCache``): a shallow forward replays the tail of a full one bit for bit,
matches the CPU oracle's statement of the rule (tests/deepcache_oracle.py) at another input, runs only the layers it should;
cached trajectories follow the oracle loop driving the wrapped oracle models, really differ from the uncached ones, batch over
requests, and the cache lives for exactly one call.  SMALL config, latent 16 x 16, 10 steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair, err_stats  # noqa: E402

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
DTYPES = dict(params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module", **DTYPES)
def pair(request):
    """engines and oracle models from one state dict, with a ControlNet; garment features harvested once on both sides"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.unet import nchw_to_nhwc8
    from oracle.pipeline import garment_features
    torch.manual_seed(0)
    dt = request.param
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dt)
    p["dtype"] = dt
    refl, cloth = g(13, 1, 4, 16, 16), g(12, 2, 16, 64, scale=0.5)
    with torch.no_grad():
        p["sa_o"] = garment_features(p["o_ref"], refl, cloth)
        p["e_ref"].forward_nhwc(nchw_to_nhwc8(refl.cuda(), dt), 0, cloth[1:2].cuda().to(dt).contiguous())
    p["sa_e"] = {n: pr.cache["hidden_states"] for n, pr in p["e_ref"].attn_processors.items()}
    return p


def _inputs(p, seed, hw=16):
    """a CFG batch of two rows: the same latent twice (what ``cfg_pair`` promises), prompt / negative context, a pose image"""
    from imagdressing_amd.unet import nchw_to_nhwc8
    lat = g(seed, 1, 4, hw, hw).repeat(2, 1, 1, 1)
    ehs = torch.cat([g(seed + 1, 1, 77, 64, scale=0.5), g(seed + 2, 1, 77, 64, scale=0.5)])
    pose = torch.rand(1, 3, 8 * hw, 8 * hw, generator=torch.Generator().manual_seed(seed + 3))
    dt = p["dtype"]
    return dict(lat=lat, ehs=ehs, pose=pose, x=nchw_to_nhwc8(lat.cuda(), dt), ehs_e=ehs.cuda().to(dt).contiguous(),
                pose_e=nchw_to_nhwc8(pose.cuda(), dt))


def _cak(p):
    return {"sa_hidden_states": p["sa_e"], "sa_batch_mask": torch.tensor([1.0, 0.0], device="cuda"), "sa_pair_layout": True}


def _engine(p, inp, t, dc, *, ctrl, cfg_pair):
    """ControlNet (optional) + UNet forward of the engines in the cache's current mode -> (eps, down residuals)"""
    down = mid = None
    if ctrl:
        down, mid = p["e_ctrl"].forward_nhwc(inp["x"], t, inp["ehs_e"], inp["pose_e"], 0.8, **({} if dc is None else {"deepcache": dc}))
    eps = p["e_unet"].forward_nhwc(inp["x"], t, inp["ehs_e"], _cak(p), down, mid, cfg_pair=cfg_pair, **({} if dc is None else {"deepcache": dc}))
    return eps, down, mid


# ---- 1. exact replay ----
@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlnet"])
@pytest.mark.parametrize("cfg_pair", [False, True], ids=["rows", "cfg_pair"])
@pytest.mark.parametrize("depth", [1, 2, 3])
@torch.no_grad()
def test_shallow_replays_the_full_forward_bit_for_bit(pair, depth, cfg_pair, ctrl):
    """A full forward that stores F_d, then a shallow one on the SAME x, t, context and residuals: the same kernels on the same bytes,
    so eps is ``torch.equal`` -- unless a skip or residual index is off, the stored feature was clobbered (an unrelated forward runs in
    between and reuses every scratch buffer), or a statistics pass is missing.  The shallow ControlNet residuals are the first d of
    the full list.  And a full forward with the cache equals the forward without one."""
    from imagdressing_amd.unet import DeepCache
    p = pair
    inp, other = _inputs(p, 100), _inputs(p, 200)
    plain, _, _ = _engine(p, inp, 481, None, ctrl=ctrl, cfg_pair=cfg_pair)
    dc = DeepCache(depth)
    full, down, mid = _engine(p, inp, 481, dc, ctrl=ctrl, cfg_pair=cfg_pair)
    assert torch.equal(full, plain)
    full, down = full.clone(), None if down is None else [d.clone() for d in down]
    _engine(p, other, 77, None, ctrl=ctrl, cfg_pair=cfg_pair)                  # churn: same shapes, other values, no cache
    dc.full = False
    shallow, sdown, smid = _engine(p, inp, 481, dc, ctrl=ctrl, cfg_pair=cfg_pair)
    assert torch.isfinite(full).all()
    assert torch.equal(shallow, full), (shallow - full).abs().max().item()
    if ctrl:
        assert smid is None and mid is not None and len(down) == 12 and len(sdown) == depth
        assert all(torch.equal(a, b) for a, b in zip(sdown, down))
    # the shallow forward does depend on the feature: another input's F_d gives another eps
    dc.full = True
    _engine(p, other, 481, dc, ctrl=ctrl, cfg_pair=cfg_pair)
    dc.full = False
    assert not torch.equal(_engine(p, inp, 481, dc, ctrl=ctrl, cfg_pair=cfg_pair)[0], full)


@torch.no_grad()
def test_shallow_replay_on_the_pair_half_path():
    """32 x 32 latents: the first hybrid block of a CFG pair runs its self-attention phase once for both halves
    (``Transformer2D.call_pair_half``, N >= 512) -- the path a depth-2 / depth-3 shallow forward takes in the sampling loop"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops
    from imagdressing_amd.unet import DeepCache, nchw_to_nhwc8
    dt = torch.float16
    p = build_pair(SMALL, seed=5, dtype=dt)
    p["dtype"] = dt
    p["e_ref"].forward_nhwc(nchw_to_nhwc8(g(13, 1, 4, 32, 32).cuda(), dt), 0, g(12, 1, 16, 64, scale=0.5).cuda().to(dt).contiguous())
    p["sa_e"] = {n: pr.cache["hidden_states"] for n, pr in p["e_ref"].attn_processors.items()}
    inp = _inputs(p, 100, hw=32)
    blk = p["e_unet"].down_blocks[0].attentions[0]
    assert ops.CFG_PAIR_ATTN and blk.pair_half_ok(torch.empty(1, 32, 32, 80, dtype=dt, device="cuda"), _cak(p))
    for depth in (2, 3):
        dc = DeepCache(depth)
        full = _engine(p, inp, 481, dc, ctrl=False, cfg_pair=True)[0].clone()
        _engine(p, _inputs(p, 200, hw=32), 77, None, ctrl=False, cfg_pair=True)
        dc.full = False
        assert torch.equal(_engine(p, inp, 481, dc, ctrl=False, cfg_pair=True)[0], full), depth


@torch.no_grad()
def test_shallow_forward_refusals(pair):
    from imagdressing_amd.unet import DeepCache
    p = pair
    inp = _inputs(p, 100)
    dc = DeepCache(1)
    dc.full = False
    with pytest.raises(ValueError, match="before any full"):
        _engine(p, inp, 481, dc, ctrl=False, cfg_pair=False)
    with pytest.raises(ValueError, match="before any full"):
        p["e_ctrl"].forward_nhwc(inp["x"], 481, inp["ehs_e"], inp["pose_e"], 0.8, deepcache=dc)
    dc.full = True
    _engine(p, inp, 481, dc, ctrl=True, cfg_pair=False)
    dc.full = False
    wide = _inputs(p, 100, hw=24)
    four = dict(inp, x=inp["x"].repeat(2, 1, 1, 1), ehs_e=inp["ehs_e"].repeat(2, 1, 1))
    for bad in (wide, four):
        with pytest.raises(ValueError, match="the cache holds"):
            _engine(p, bad, 481, dc, ctrl=False, cfg_pair=False)
        with pytest.raises(ValueError, match="the cache holds"):
            p["e_ctrl"].forward_nhwc(bad["x"], 481, bad["ehs_e"], bad["pose_e"], 0.8, deepcache=dc)
    dc.depth = 2
    with pytest.raises(ValueError, match="the cache holds"):
        _engine(p, inp, 481, dc, ctrl=False, cfg_pair=False)
    dc.depth = 4
    with pytest.raises(ValueError, match=r"1 \.\. 3"):
        _engine(p, inp, 481, dc, ctrl=False, cfg_pair=False)


# ---- 2. shallow forward against the oracle, at another input ----
@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlnet"])
@pytest.mark.parametrize("depth", [1, 2, 3])
@torch.no_grad()
def test_shallow_forward_matches_oracle(pair, depth, ctrl):
    """F_d from (x, t), the shallow forward at (x', t'): against the oracle's sub-modules applying the same rule, within the bars of
    one SMALL UNet forward (test_e2e_gpu.BARS)"""
    from imagdressing_amd.unet import DeepCache
    from tests.deepcache_oracle import controlnet_forward, unet_forward
    from tests.test_e2e_gpu import BARS
    p = pair
    a, b = _inputs(p, 100), _inputs(p, 300)
    ta, tb = 481, 441
    dc = DeepCache(depth)
    _engine(p, a, ta, dc, ctrl=ctrl, cfg_pair=True)
    dc.full = False
    got, _, _ = _engine(p, b, tb, dc, ctrl=ctrl, cfg_pair=True)
    # the oracle: cond row with the garment, uncond row without (the loop's two batch-1 calls), each stream with its own F_d
    refs = []
    for row, cak in ((0, {"sa_hidden_states": p["sa_o"]}), (1, None)):
        sl = slice(row, row + 1)
        down_a = mid_a = down_b = None
        if ctrl:
            down_a, mid_a = controlnet_forward(p["o_ctrl"], a["lat"][sl], ta, a["ehs"][sl], a["pose"], 0.8)
            down_b, none = controlnet_forward(p["o_ctrl"], b["lat"][sl], tb, b["ehs"][sl], b["pose"], 0.8, depth)
            assert none is None and len(down_b) == depth
        _, feat = unet_forward(p["o_unet"], a["lat"][sl], ta, a["ehs"][sl], cak, down_a, mid_a, depth)
        eps, _ = unet_forward(p["o_unet"], b["lat"][sl], tb, b["ehs"][sl], cak, down_b, None, depth, feat=feat)
        refs.append(eps)
    ref = torch.cat(refs)
    st = err_stats(got.view(2, 16, 16, 4).permute(0, 3, 1, 2), ref)
    print(f"shallow_forward_vs_oracle[{p['dtype']}, depth {depth}, ctrl {ctrl}]: {st}")
    bar = BARS[p["dtype"]]
    assert st["max_abs"] < bar["max_abs"] and st["rel_rms"] < bar["rel_rms"], st


# ---- 3. only the intended layers run ----
@pytest.mark.parametrize("cfg_pair", [False, True], ids=["rows", "cfg_pair"])
@pytest.mark.parametrize("depth", [1, 2, 3])
@torch.no_grad()
def test_only_the_intended_processors_run(pair, depth, cfg_pair):
    from imagdressing_amd.unet import DeepCache
    p = pair
    inp = _inputs(p, 100)
    procs = p["e_unet"].attn_processors
    seen = []
    saved = {}
    for name, proc in procs.items():
        saved[name] = proc.__class__

        def rec(self, *a, _name=name, _base=proc.__class__, **k):
            seen.append(_name)
            return _base.__call__(self, *a, **k)
        proc.__class__ = type("Recorded" + saved[name].__name__, (saved[name],), {"__call__": rec})
    try:
        dc = DeepCache(depth)
        _engine(p, inp, 481, dc, ctrl=False, cfg_pair=cfg_pair)
        assert set(seen) == set(procs) and len(seen) == len(procs)          # a full forward runs all 32, once each
        seen.clear()
        dc.full = False
        _engine(p, inp, 481, dc, ctrl=False, cfg_pair=cfg_pair)
    finally:
        for name, proc in procs.items():
            proc.__class__ = saved[name]
    want = []
    for j in range(depth - 1):
        want += [f"down_blocks.0.attentions.{j}.transformer_blocks.0.attn{a}.processor" for a in (1, 2)]
    for j in range(3 - depth, 3):
        want += [f"up_blocks.3.attentions.{j}.transformer_blocks.0.attn{a}.processor" for a in (1, 2)]
    assert seen == want, (depth, seen)


# ---- pipelines ----
def _sched(name):
    from imagdressing_amd import scheduler as S
    return {"ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW),
            "dpm": lambda: S.DPMSolverMultistepScheduler(**KW),
            "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW),
            "unipc": lambda: S.UniPCMultistepScheduler(**KW)}[name]()


def _sched_oracle(name):
    from oracle.ddim import DDIMOracle
    from oracle.unipc import UniPCOracle
    from tests.sampler_oracle import DPMSolverOracle, PNDMOracle
    return {"ddim": DDIMOracle, "dpm": DPMSolverOracle, "pndm": PNDMOracle, "unipc": UniPCOracle}[name]()


STEPS, GS = 10, 7.0
PE, NE = g(10, 1, 77, 64, scale=0.5), g(11, 1, 77, 64, scale=0.5)
CLOTH, REFL = g(12, 2, 16, 64, scale=0.5), g(13, 1, 4, 16, 16)
LAT = g(42, 1, 4, 16, 16)


def _base_pipe(p, name="ddim"):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    return IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           image_encoder=None, ImgProj=lambda h: h, scheduler=_sched(name), safety_checker=None, feature_extractor=None)


def _base_kw(lat=LAT, steps=STEPS, **over):
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=steps,
              guidance_scale=GS, num_images_per_prompt=lat.shape[0], prompt_embeds=PE.cuda(), negative_prompt_embeds=NE.cuda(),
              ref_clip_hidden_states=CLOTH[1:2].cuda(), ref_image_latents=REFL.cuda(), latents=lat.cuda(), output_type="latent")
    kw.update(over)
    return kw


_ORACLE = {}


def _oracle_base(p, name, interval, depth):
    """oracle.pipeline.denoise driving the wrapped oracle UNet (fp32 on the CPU: one run serves both element types);
    interval 1 = the plain oracle UNet"""
    key = (name, interval, depth)
    if key not in _ORACLE:
        from oracle.pipeline import denoise
        from tests.deepcache_oracle import DeepCacheUNet
        orc = _sched_oracle(name)
        orc.set_timesteps(STEPS)
        unet = p["o_unet"] if interval == 1 else DeepCacheUNet(p["o_unet"], interval, depth, n_calls=STEPS + 1)
        _ORACLE[key] = denoise(unet, p["o_ref"], orc, LAT * getattr(orc, "init_noise_sigma", 1.0), PE, NE, CLOTH, REFL, STEPS, GS)
        if interval > 1:
            calls = STEPS + 1 if name == "pndm" else STEPS            # PNDM's extra call is one more index of the plan
            assert unet.n == 2 * calls and not all(unet.modes)
    return _ORACLE[key]


def _check_traj(out, ref, dtype, what):
    from tests.test_e2e_gpu import _traj_bar
    st = err_stats(out, ref)
    print(f"{what}[{dtype}]: {st}")
    bar = _traj_bar(dtype)
    assert torch.isfinite(out).all()
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st
    return st


# ---- 4. trajectories ----
@pytest.mark.parametrize("interval,depth", [(3, 1), (2, 2)])
@pytest.mark.parametrize("name", ["ddim", "dpm", "pndm", "unipc"])
@torch.no_grad()
def test_cached_trajectory_matches_oracle(pair, name, interval, depth):
    """the three UNet call sites of the loop: the DDIM step, the fused sampler step (DPM-Solver++; PNDM with its extra call), UniPC"""
    p = pair
    pipe = _base_pipe(p, name).enable_deepcache(cache_interval=interval, depth=depth)
    trace = []
    out = pipe(trace=trace, **_base_kw()).images
    assert len(trace) == (STEPS + 1 if name == "pndm" else STEPS)
    _check_traj(out, _oracle_base(p, name, interval, depth), p["dtype"], f"deepcache_{name}_{interval}_{depth}")


@pytest.mark.parametrize("interval,depth", [(3, 1), (2, 2)])
@torch.no_grad()
def test_cached_controlnet_trajectory_matches_oracle(pair, interval, depth):
    """the ControlNet pipeline: the ControlNet call of a step runs in the UNet call's mode and hands over d residuals"""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    from tests.deepcache_oracle import DeepCacheControlNet, DeepCacheUNet
    p = pair
    pose = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16))
    key = ("controlnet", interval, depth)
    if key not in _ORACLE:
        _ORACLE[key] = denoise(DeepCacheUNet(p["o_unet"], interval, depth, STEPS), p["o_ref"], DDIMOracle(), LAT, PE, NE, CLOTH, REFL, STEPS, GS,
                               controlnet=DeepCacheControlNet(p["o_ctrl"], interval, depth, STEPS), control_image=pose,
                               prompt_embeds_control=torch.cat([NE, PE]), conditioning_scale=0.8)
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched("ddim"))
    pipe.enable_deepcache(cache_interval=interval, depth=depth)
    out = pipe(pose_image=pose.cuda(), controlnet_conditioning_scale=0.8, **_base_kw()).images
    _check_traj(out, _ORACLE[key], p["dtype"], f"deepcache_controlnet_{interval}_{depth}")


@pytest.mark.parametrize("interval,depth", [(3, 1), (2, 2)])
@torch.no_grad()
def test_cached_inpainting_trajectory_matches_oracle(pair, interval, depth):
    """the inpainting pipeline, blend plus strength = 0.6: 6 of 10 timesteps run, and the plan counts from the first executed one"""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    from tests.deepcache_oracle import DeepCacheControlNet, DeepCacheUNet
    p = pair
    strength = 0.6
    noise, img_lat = g(42, 1, 4, 16, 24), g(17, 1, 4, 16, 24)
    mask = torch.zeros(1, 1, 16, 24); mask[:, :, 4:12, 6:18] = 1.0
    ctrl = torch.rand(1, 3, 128, 192, generator=torch.Generator().manual_seed(18))
    key = ("inpaint", interval, depth)
    if key not in _ORACLE:
        unet = DeepCacheUNet(p["o_unet"], interval, depth, STEPS)
        _ORACLE[key] = denoise(unet, p["o_ref"], DDIMOracle(), None, PE, NE, CLOTH, REFL, STEPS, 5.0,
                               controlnet=DeepCacheControlNet(p["o_ctrl"], interval, depth, STEPS), control_image=ctrl,
                               prompt_embeds_control=torch.cat([NE, PE]), conditioning_scale=1.0,
                               inpaint=dict(mask=mask, image_latents=img_lat, noise=noise), strength=strength)
        assert unet.n == 12 and unet.modes[:2] == [True, True]
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched("ddim"))
    pipe.enable_deepcache(cache_interval=interval, depth=depth)
    mine = []
    out = pipe(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=192, height=128, num_inference_steps=STEPS,
               guidance_scale=5.0, control_image=ctrl.cuda(), prompt_embeds=PE.cuda(), negative_prompt_embeds=NE.cuda(),
               ref_clip_hidden_states=CLOTH[1:2].cuda(), ref_image_latents=REFL.cuda(), image_latents=img_lat.cuda(),
               mask_latents=mask.cuda(), noise=noise.cuda(), output_type="latent", strength=strength, trace=mine).images
    assert len(mine) == 6
    _check_traj(out, _ORACLE[key], p["dtype"], f"deepcache_inpaint_{interval}_{depth}")
    keep = (mask == 0).expand(1, 4, -1, -1)
    assert torch.allclose(out.cpu()[keep], img_lat[keep], atol=1e-5)


# ---- 5. the cache is really used ----
@pytest.mark.parametrize("name", ["ddim", "dpm"])
@torch.no_grad()
def test_cache_changes_the_trajectory_and_interval_one_does_not(pair, name):
    """cache_interval = 3 moves the result away from the switch-off trajectory by more than 10x its own parity error against the
    cached oracle (the device of the eta test); cache_interval = 1 is the switch-off loop, bit for bit"""
    p = pair
    pipe = _base_pipe(p, name)
    off = pipe(**_base_kw()).images
    pipe.enable_deepcache(cache_interval=1)
    assert torch.equal(pipe(**_base_kw()).images, off)
    pipe.enable_deepcache(cache_interval=3, depth=1)
    on = pipe(**_base_kw()).images
    pipe.disable_deepcache()
    assert torch.equal(pipe(**_base_kw()).images, off)
    parity = err_stats(on, _oracle_base(p, name, 3, 1))["rel_rms"]
    moved = err_stats(on, off)["rel_rms"]
    print(f"deepcache_{name}_3_1[{p['dtype']}]: parity {parity:.3e}, distance from the uncached trajectory {moved:.3e}")
    assert moved > 10 * parity, (moved, parity)


# ---- 6. request batch ----
@torch.no_grad()
def test_two_requests_batched_match_solo_calls(pair):
    """R = 2 requests (two garments, two prompts, two guidance scales) in one call with the switch on -- the cache simply holds
    2 R n rows -- against two solo calls with the switch on: the comparison and bars of test_batched_matches_solo_calls"""
    from tests.test_multi_request_gpu import _bar_small, _check, _Requests
    p, reqs = pair, _Requests(R=2)
    pipe = _base_pipe(p).enable_deepcache(cache_interval=3, depth=2)
    out = pipe(num_inference_steps=STEPS, **reqs.call_kwargs(n=2)).images
    assert out.shape == (4, 4, 16, 16)
    for r in range(2):
        solo = pipe(num_inference_steps=STEPS, **reqs.solo_kwargs(r, n=2)).images
        st = _check(out[2 * r:2 * r + 2], solo, _bar_small(p["dtype"]))
        print(f"deepcache batched vs solo, request {r} [{p['dtype']}]: {st}")
    assert not torch.equal(out[:2], out[2:])


# ---- 7. lifetime ----
@torch.no_grad()
def test_cache_lives_for_one_call(pair):
    p = pair
    pipe = _base_pipe(p).enable_deepcache(cache_interval=3, depth=1)
    lat2 = torch.cat([LAT, g(43, 1, 4, 16, 16)])
    one = pipe(**_base_kw()).images
    two = pipe(**_base_kw(lat=lat2)).images                    # another batch size right after: nothing of the first call is left
    again = pipe(**_base_kw()).images
    assert two.shape == (2, 4, 16, 16) and torch.isfinite(two).all() and torch.equal(again, one)
    fresh = _base_pipe(p).enable_deepcache(cache_interval=3, depth=1)(**_base_kw()).images
    assert torch.equal(fresh, one)

    class Boom(Exception):
        pass

    def callback(i, t, z):
        if i == 4:                                             # between a shallow call and the next full one
            raise Boom()
    with pytest.raises(Boom):
        pipe(callback=callback, **_base_kw(lat=lat2))
    assert torch.equal(pipe(**_base_kw()).images, fresh)       # the next call starts from nothing, like a fresh pipeline
    assert p["e_unet"].__dict__.get("_temb_table") is None


@pytest.mark.parametrize("name", ["ddim", "dpm"])
@torch.no_grad()
def test_step_graph_is_ignored_while_the_switch_is_on(pair, name):
    p = pair
    pipe = _base_pipe(p, name).enable_deepcache(cache_interval=3, depth=1)
    eager = pipe(**_base_kw()).images
    pipe.enable_step_graph(True)
    try:
        both = pipe(**_base_kw()).images
        assert getattr(pipe, "_last_step_graph", None) is None          # the call ran eagerly
    finally:
        pipe.enable_step_graph(False)
    assert torch.isfinite(eager).all() and torch.equal(both, eager)
