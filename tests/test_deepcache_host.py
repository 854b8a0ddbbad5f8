"""Host side of DeepCache (``enable_deepcache``): the call plan, the switch's refusals, which ControlNet residuals a shallow UNet
forward asks for, what ``_denoise`` hands the UNet with the switch off and on, and the oracle wrapper the GPU tests compare with.
Nothing here touches a GPU: the engine's launches are replaced by stand-ins that pass their input through."""
import pytest
import torch

from imagdressing_amd.dressing_sd.pipelines._base import PipelineBase, deepcache_plan


@pytest.mark.parametrize("n_calls", [1, 4, 21])
@pytest.mark.parametrize("interval", [1, 2, 3, 5])
def test_deepcache_plan(interval, n_calls):
    plan = deepcache_plan(n_calls, interval)
    assert len(plan) == n_calls and all(isinstance(f, bool) for f in plan)
    assert plan[0] is True                                            # call 0 is always full
    assert [c for c, f in enumerate(plan) if f] == list(range(0, n_calls, interval))
    assert sum(plan) == (n_calls + interval - 1) // interval
    if interval == 1:
        assert all(plan)


def test_deepcache_plan_spelled_out():
    assert deepcache_plan(4, 3) == [True, False, False, True]
    assert deepcache_plan(7, 2) == [True, False, True, False, True, False, True]          # (e.g. PNDM: 6 steps, 7 UNet calls)
    assert deepcache_plan(0, 3) == []
    for bad in (0, -1):
        with pytest.raises(ValueError, match="cache_interval"):
            deepcache_plan(4, bad)


class _RecordingUNet:
    """stand-in for the engine UNet: records the keywords of every forward and the cache's mode at that moment"""
    dtype = torch.float16
    device = torch.device("cpu")

    def __init__(self, fail_at=None):
        self.calls, self.fail_at = [], fail_at

    def forward_nhwc(self, x, t, ehs, cak, down=None, mid=None, **kw):
        dc = kw.get("deepcache")
        self.calls.append(dict(kw=dict(kw), full=None if dc is None else dc.full, depth=None if dc is None else dc.depth, cache=dc))
        if self.fail_at is not None and len(self.calls) - 1 == self.fail_at:
            raise RuntimeError("stand-in failure")
        return torch.zeros(x.shape[0], x.shape[1] * x.shape[2], 4)


def _pipe(unet, sched="ddim"):
    pipe = PipelineBase()
    from imagdressing_amd import scheduler as S
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    sch = {"ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kw),
           "dpm": lambda: S.DPMSolverMultistepScheduler(**kw), "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **kw),
           "unipc": lambda: S.UniPCMultistepScheduler(**kw)}[sched]()
    pipe._init_common(vae=None, reference_unet=None, unet=unet, tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None,
                      scheduler=sch)
    return pipe


def _run(pipe, steps=7, **kw):
    return pipe._denoise(latents=torch.zeros(1, 4, 4, 4), prompt_embeds=torch.zeros(1, 3, 8), negative_prompt_embeds=torch.zeros(1, 3, 8),
                         sa_hidden_states={}, num_inference_steps=steps, guidance_scale=7.5, **kw)


@pytest.fixture
def no_launches(monkeypatch):
    """the scheduler steps are launches: here they leave the latent alone"""
    from imagdressing_amd import ops
    monkeypatch.setattr(ops, "ddim_cfg_step", lambda *a, **k: None)
    monkeypatch.setattr(ops, "sampler_step", lambda *a, **k: None)
    monkeypatch.setattr(ops, "lincomb", lambda terms, out=None: out if out is not None else terms[0][1].clone())
    monkeypatch.setattr(ops, "workspace", lambda tag, shape, dtype, device, init=None: torch.zeros(tuple(shape), dtype=dtype))


def test_enable_deepcache_refusals():
    pipe = _pipe(_RecordingUNet())
    for bad in (0, -2):
        with pytest.raises(ValueError, match="cache_interval"):
            pipe.enable_deepcache(cache_interval=bad)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match=r"1 \.\. 3"):             # layers_per_block + 1 = 3 for SD1.5
            pipe.enable_deepcache(depth=bad)
    assert getattr(pipe, "_deepcache", None) is None                  # a refused call leaves the switch off
    assert pipe.enable_deepcache() is pipe and pipe._deepcache == (3, 1)
    assert pipe.enable_deepcache(cache_interval=5, depth=3)._deepcache == (5, 3)
    assert pipe.disable_deepcache() is pipe and pipe._deepcache is None


def test_all_four_pipelines_have_the_switch():
    import importlib
    for mod in ("IMAGDressing_v1_pipeline", "IMAGDressing_v1_pipeline_controlnet", "IMAGDressing_v1_pipeline_controlnet_inpainting",
                "IMAGDressing_v1_pipeline_ipa_controlnet"):
        cls = importlib.import_module("imagdressing_amd.dressing_sd.pipelines." + mod).IMAGDressing_v1
        assert callable(cls.enable_deepcache) and callable(cls.disable_deepcache) and callable(cls.enable_step_graph)


def test_switch_off_passes_no_cache_keyword(no_launches):
    unet = _RecordingUNet()
    pipe = _pipe(unet)
    _run(pipe)
    assert len(unet.calls) == 7 and all(c["kw"] == {"cfg_pair": True} for c in unet.calls)
    # interval 1 computes what the switch-off loop computes: the same calls, no keyword
    unet.calls.clear()
    pipe.enable_deepcache(cache_interval=1)
    _run(pipe)
    assert len(unet.calls) == 7 and all(c["kw"] == {"cfg_pair": True} for c in unet.calls)
    # ... and off again after disable_deepcache
    unet.calls.clear()
    pipe.enable_deepcache(cache_interval=3).disable_deepcache()
    _run(pipe)
    assert all(c["kw"] == {"cfg_pair": True} for c in unet.calls)


@pytest.mark.parametrize("sched", ["ddim", "dpm", "pndm", "unipc"])
@pytest.mark.parametrize("interval,depth", [(3, 1), (2, 2), (5, 3)])
def test_switch_on_follows_the_plan(no_launches, interval, depth, sched):
    """all three UNet call sites of the loop -- the DDIM step, the fused sampler step (PNDM: one call more than steps), UniPC"""
    unet = _RecordingUNet()
    pipe = _pipe(unet, sched)
    pipe.enable_deepcache(cache_interval=interval, depth=depth)
    _run(pipe)
    n = 8 if sched == "pndm" else 7
    assert len(unet.calls) == n and [c["full"] for c in unet.calls] == deepcache_plan(n, interval)
    assert all(c["depth"] == depth for c in unet.calls)
    caches = {id(c["cache"]) for c in unet.calls}
    assert len(caches) == 1                                           # one cache per call of the loop ...
    first = unet.calls[0]["cache"]
    unet.calls.clear()
    _run(pipe)
    assert unet.calls[0]["cache"] is not first and unet.calls[0]["full"] is True          # ... and a new one for the next


def test_strength_counts_from_the_first_executed_call(no_launches):
    unet = _RecordingUNet()
    pipe = _pipe(unet)
    pipe.enable_deepcache(cache_interval=3)
    _run(pipe, steps=10, t_start=4)
    assert [c["full"] for c in unet.calls] == [True, False, False, True, False, False]


def test_cache_is_dropped_when_the_loop_raises(no_launches):
    from imagdressing_amd.unet import DeepCache
    unet = _RecordingUNet(fail_at=2)
    pipe = _pipe(unet)
    pipe.enable_deepcache(cache_interval=3)
    dropped = []
    real_clear = DeepCache.clear

    def clear(self):
        dropped.append(self)
        real_clear(self)
    DeepCache.clear = clear
    try:
        with pytest.raises(RuntimeError, match="stand-in failure"):
            _run(pipe)
    finally:
        DeepCache.clear = real_clear
    assert dropped == [unet.calls[0]["cache"]] and dropped[0]._feat is None and dropped[0]._sig is None


def test_cache_refuses_mismatched_calls():
    """shallow before full, and a stored feature of another batch / size / dtype / depth: ValueError (no launch needed to find out)"""
    from imagdressing_amd.unet import DeepCache
    x = torch.zeros(2, 4, 6, 8, dtype=torch.float16)
    dc = DeepCache(2)
    with pytest.raises(ValueError, match="before any full"):
        dc.load(x)
    with pytest.raises(ValueError, match="before any full"):
        dc.check_controlnet(x)
    dc._feat, dc._sig = torch.zeros(2, 4, 6, 16, dtype=torch.float16), DeepCache._signature(x, 2)      # what store() leaves behind
    dc.note_controlnet(x)
    assert dc.load(x) is dc._feat
    dc.check_controlnet(x)
    for other in (torch.zeros(4, 4, 6, 8, dtype=torch.float16), torch.zeros(2, 6, 6, 8, dtype=torch.float16),
                  torch.zeros(2, 4, 8, 8, dtype=torch.float16), torch.zeros(2, 4, 6, 8, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="the cache holds"):
            dc.load(other)
        with pytest.raises(ValueError, match="the cache holds"):
            dc.check_controlnet(other)
    dc.depth = 1
    with pytest.raises(ValueError, match="the cache holds"):
        dc.load(x)
    for bad in (0, 4):
        with pytest.raises(ValueError, match=r"1 \.\. 3"):
            DeepCache(bad).check_depth(2)


class _Indices(list):
    """a residual list that records which entries are read"""

    def __init__(self, n):
        super().__init__([None] * n)
        self.read = []

    def __getitem__(self, i):
        self.read.append(i)
        return None


@pytest.fixture
def passthrough_engine(monkeypatch):
    """the engine UNet of the SMALL config on the CPU with every launch replaced by a pass-through: what is left is the control flow
    of ``forward_nhwc`` -- which layers run and which residuals they ask for"""
    from imagdressing_amd import ops
    from imagdressing_amd import unet as E
    from tests.harness import SMALL
    ran = []
    monkeypatch.setattr(E.ResnetBlock, "__call__", lambda self, x, temb: ran.append(self) or x)
    monkeypatch.setattr(E.Transformer2D, "__call__", lambda self, x, ehs, cak: ran.append(self) or x)
    monkeypatch.setattr(E.ConvOp, "__call__", lambda self, x, **kw: (ran.append(self) or x) if not kw.get("out_f32")
                        else (ran.append(self) or torch.zeros(x.shape[:-1] + (4,))))
    monkeypatch.setattr(E._Encoder, "_time_embed", lambda self, t, B, dev: None)
    monkeypatch.setattr(ops, "concat_channels", lambda a, b, c=None, gn_stats_groups=0: a)
    monkeypatch.setattr(ops, "group_norm", lambda x, *a, **k: x)
    monkeypatch.setattr(ops, "add", lambda a, b, *r, **k: a)
    monkeypatch.setattr(ops, "repeat_batch", lambda x, times=2: torch.cat([x] * times))
    monkeypatch.setattr(ops, "copy_into", lambda dst, src: dst.copy_(src))
    full = dict(E.SD15_CONFIG, **SMALL)
    unet = E.UNet2DConditionModel(E.random_state_dict(E.unet_param_shapes(full), 0), SMALL, "cpu", torch.float16)
    return unet, ran


@pytest.mark.parametrize("cfg_pair", [False, True], ids=["plain", "cfg_pair"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_controlnet_residual_indices_per_depth(passthrough_engine, depth, cfg_pair):
    """layer j of the last up block consumes skip L - j and the ControlNet residual of the same index (``ctrl[len(skips)]``): a
    shallow forward at depth d asks for residuals d - 1 .. 0, a full one for 11 .. 0"""
    from imagdressing_amd.unet import DeepCache
    unet, ran = passthrough_engine
    x = torch.zeros(2, 4, 4, 8, dtype=torch.float16)
    dc = DeepCache(depth)
    ctrl = _Indices(12)
    unet.forward_nhwc(x, 10, None, None, ctrl, None, cfg_pair=cfg_pair, deepcache=dc)
    assert ctrl.read == list(range(11, -1, -1))
    assert dc._feat is not None and dc._sig == (2, 4, 4, torch.float16, depth)
    n_full = len(ran)
    ran.clear()
    dc.full = False
    ctrl = _Indices(depth)
    eps = unet.forward_nhwc(x, 10, None, None, ctrl, None, cfg_pair=cfg_pair, deepcache=dc)
    assert eps.shape == (2, 16, 4)
    assert ctrl.read == list(range(depth - 1, -1, -1))
    # the layers that ran: conv_in, layers 0 .. d-2 of down_blocks[0], layers 3-d .. 2 of the last up block, conv_out -- nothing else
    d0, up = unet.down_blocks[0], unet.up_blocks[-1]
    want = [unet.conv_in]
    for j in range(depth - 1):
        want += [d0.resnets[j], d0.attentions[j]]
    for j in range(3 - depth, 3):
        want += [up.resnets[j], up.attentions[j]]
    want.append(unet.conv_out)
    assert [id(m) for m in ran] == [id(m) for m in want] and len(ran) < n_full


def test_oracle_wrapper_full_call_is_the_oracle_forward():
    """tests/deepcache_oracle.py: its full forward is the oracle's own (bit for bit), F_d is what enters the cut layer, and a shallow
    forward on the same input reproduces the full one (fp32 on one machine: the same operations on the same values)"""
    from oracle import sd15
    from tests.deepcache_oracle import DeepCacheControlNet, DeepCacheUNet, controlnet_forward, unet_forward
    from tests.harness import SMALL, oracle_cfg
    torch.manual_seed(0)
    m = sd15.UNet2DConditionModel(oracle_cfg(SMALL)).eval()
    c = sd15.ControlNetModel(oracle_cfg(SMALL)).eval()
    g = torch.Generator().manual_seed(1)
    x, ehs = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 5, 64, generator=g)
    cond = torch.rand(2, 3, 64, 64, generator=g)
    with torch.no_grad():
        down, mid = c(x, 400, ehs, cond, 0.7)
        ref = m(x, 400, ehs, down_block_additional_residuals=down, mid_block_additional_residual=mid)
        for depth in (1, 2, 3):
            eps, feat = unet_forward(m, x, 400, ehs, None, down, mid, depth)
            assert torch.equal(eps, ref)
            sdown, smid = controlnet_forward(c, x, 400, ehs, cond, 0.7, depth)
            assert smid is None and len(sdown) == depth and all(torch.equal(a, b) for a, b in zip(sdown, down))
            eps_s, _ = unet_forward(m, x, 400, ehs, None, sdown, None, depth, feat=feat)
            assert torch.allclose(eps_s, ref, rtol=0, atol=1e-5)
        # the callables follow the plan, one F_d per stream
        w = DeepCacheUNet(m, 2, 1, n_calls=3, streams=2)
        outs = [w(x[i % 2:i % 2 + 1], 400, ehs[i % 2:i % 2 + 1]) for i in range(6)]
        assert w.modes == [True, True, False, False, True, True]
        assert torch.allclose(outs[2], outs[0], atol=1e-5) and torch.allclose(outs[3], outs[1], atol=1e-5)
        assert not torch.allclose(outs[0], outs[1], atol=1e-3)
        wc = DeepCacheControlNet(c, 2, 2, n_calls=2)
        d0, m0 = wc(x, 400, ehs, cond, 0.7)
        d1, m1 = wc(x, 400, ehs, cond, 0.7)
        assert len(d0) == 12 and torch.is_tensor(m0) and len(d1) == 2 and m1 == (None, None)
