"""``enable_request_adapter_scales`` on the GPU: ``ipa_scale``, ``s_lora_scale`` and ``c_lora_scale`` per request in ONE call of the
IP-Adapter + ControlNet pipeline -- the LoRA of the rows' layers unfolded (``imd_lora_expand_rows``), the face-token weight per row --
against independent fp32 runs of the reference loop (oracle.pipeline.denoise at batch 1) with the oracle processors' ``scale`` /
``lora_scale`` set to each request's values.  The bar is the one of the existing two-request IP-Adapter test
(tests/test_multi_request_gpu.py: ``_traj_bar(dtype)``, ``floor=1.0``): the unfolded route gets no wider one.

The harness's own LoRA fill is strong enough for the swap test: with the oracle alone, swapping the triples of requests 0 and 1 moves the
final latents by rel_rms 0.85 / 0.58 (max 35 / 28 at a latent scale of 12), far above four times either bar -- asserted on the CPU below."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair, err_stats  # noqa: E402
from tests.test_multi_request_gpu import _Requests, _check, _sched, _traj_bar, g  # noqa: E402

# (ipa_scale, s_lora_scale, c_lora_scale) of requests 0, 1, 2; the third is the reference's no-face setting
TRIPLES = ((0.9, 0.2, 0.2), (0.3, 0.8, 0.0), (0.0, 0.0, 0.0))
GUIDANCE = (7.0, 5.5, 6.5)
STEPS = 8
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")

FACE_P = [g(80 + r, 1, 4, 64, scale=0.5) for r in range(3)]
FACE_N = [g(90 + r, 1, 4, 64, scale=0.5) for r in range(3)]
POSE = [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r)) for r in range(3)]


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def pair(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    p = build_pair(SMALL, seed=3, kind="ipa", with_controlnet=True, dtype=request.param)
    p["dtype"] = request.param
    return p


def _set_oracle(o_unet, triple):
    ipa, s_lora, c_lora = triple
    for name, proc in o_unet.attn_processors.items():
        if name.endswith("attn1.processor"):
            proc.lora_scale = s_lora
        else:
            proc.scale, proc.lora_scale = ipa, c_lora


_ORACLE = {}          # fp32 on the CPU from one seeded state dict: one run serves both element types


def _oracle(p, reqs, r, triple, i=0, deepcache=None, sched="ddim"):
    """the reference loop for image i of request r with the processors at ``triple``"""
    key = (r, i, tuple(triple), deepcache, sched)
    if key not in _ORACLE:
        from oracle.ddim import DDIMOracle
        from oracle.pipeline import denoise
        unet, ctrl = p["o_unet"], p["o_ctrl"]
        if deepcache is not None:
            from tests.deepcache_oracle import DeepCacheControlNet, DeepCacheUNet
            unet, ctrl = DeepCacheUNet(unet, deepcache[0], deepcache[1], STEPS), DeepCacheControlNet(ctrl, deepcache[0], deepcache[1], STEPS)
        _set_oracle(p["o_unet"], triple)
        try:
            _ORACLE[key] = denoise(unet, p["o_ref"], DDIMOracle(), reqs.latent(r, i), torch.cat([reqs.pe[r], FACE_P[r]], 1),
                                   torch.cat([reqs.ne[r], FACE_N[r]], 1), reqs.cloth[r], reqs.refl[r], STEPS, GUIDANCE[r], controlnet=ctrl,
                                   control_image=POSE[r], prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]), conditioning_scale=0.8)
        finally:
            _set_oracle(p["o_unet"], (0.9, 0.2, 0.2))
    return _ORACLE[key]


class FaceProj:      # image_proj_model stand-in: the face clip hidden states carry the request index (+ r + 1 cond, -(r + 1) uncond)
    def __call__(self, idv, clip):
        idx = clip[:, 0, 0].round().long().tolist()
        return torch.cat([FACE_P[i - 1] if i > 0 else FACE_N[-i - 1] for i in idx]).cuda()


def _pipe(p, scheduler=None):
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_ipa_controlnet import IMAGDressing_v1
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, ip_ckpt=None, scheduler=scheduler or _sched())
    pipe.image_proj_model = FaceProj()
    return pipe


def _call_kw(reqs, triples, n=1):
    R = reqs.R
    fc, fu = torch.zeros(R, 257, 1280), torch.zeros(R, 257, 1280)
    for r in range(R):
        fc[r, 0, 0], fu[r, 0, 0] = r + 1, -(r + 1)
    kw = reqs.call_kwargs(n=n, guidance=GUIDANCE, image_scale=(1.0,) * R)
    kw.update(num_inference_steps=STEPS, pose_image=[POSE[r].cuda() for r in range(R)], faceid_embeds=torch.ones(R, 512),
              face_clip_hidden_states=fc, face_uncond_clip_hidden_states=fu, controlnet_conditioning_scale=0.8,
              ipa_scale=[t[0] for t in triples[:R]], s_lora_scale=[t[1] for t in triples[:R]], c_lora_scale=[t[2] for t in triples[:R]])
    return kw


def _passes(out, ref, dtype):
    st, bar = err_stats(out, ref), _traj_bar(dtype)
    return st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], st


@torch.no_grad()
def test_three_requests_match_oracle_and_swapped_scales_do_not(pair):
    """R = 3 distinct triples in one call: every row against the oracle's solo run at ITS triple (the third: all zero, the
    reference's no-face settings) -- and against the runs with the triples of requests 0 and 1 SWAPPED the same output must fail"""
    from imagdressing_amd import ops
    p, reqs = pair, _Requests(R=3)
    own = [_oracle(p, reqs, r, TRIPLES[r]) for r in range(3)]
    swapped = [_oracle(p, reqs, 0, TRIPLES[1]), _oracle(p, reqs, 1, TRIPLES[0])]
    bar = _traj_bar(p["dtype"])
    for r in range(2):          # on the CPU, oracle alone: the swap moves the final latents by at least 4x the bar
        st = err_stats(swapped[r], own[r])
        print(f"oracle, request {r}, swapped triple vs own: {st}")
        assert st["max_abs"] >= 4 * bar["max_abs"] * max(st["ref_std"], 1.0) or st["rel_rms"] >= 4 * bar["rel_rms"], st
    before = ops.LORA_ROWS_COUNTER["launches"]
    out = _pipe(p).enable_request_adapter_scales()(**_call_kw(reqs, TRIPLES)).images
    assert out.shape == (3, 4, 16, 16)
    assert ops.LORA_ROWS_COUNTER["launches"] > before          # the unfolded route ran
    for r in range(3):
        st = _check(out[r:r + 1], own[r], bar, floor=1.0)
        print(f"request {r} [{p['dtype']}]: {st}")
    for r in range(2):
        ok, st = _passes(out[r:r + 1], swapped[r], p["dtype"])
        print(f"request {r} against the swapped oracle [{p['dtype']}]: {st}")
        assert not ok, st


@torch.no_grad()
def test_two_images_per_request_carry_the_request_scales(pair):
    p, reqs = pair, _Requests(R=2)
    out = _pipe(p).enable_request_adapter_scales()(**_call_kw(reqs, TRIPLES, n=2)).images
    assert out.shape == (4, 4, 16, 16)
    for r in range(2):
        for i in range(2):
            st = _check(out[2 * r + i:2 * r + i + 1], _oracle(p, reqs, r, TRIPLES[r], i), _traj_bar(p["dtype"]), floor=1.0)
            print(f"request {r} image {i} [{p['dtype']}]: {st}")


@torch.no_grad()
def test_equal_values_keep_the_folded_route_bit_for_bit(pair):
    from imagdressing_amd import ops
    p, reqs = pair, _Requests(R=2)
    kw = _call_kw(reqs, (TRIPLES[0], TRIPLES[0]))
    off = dict(kw, ipa_scale=TRIPLES[0][0], s_lora_scale=TRIPLES[0][1], c_lora_scale=TRIPLES[0][2])
    ref = _pipe(p)(**off).images
    before = ops.LORA_ROWS_COUNTER["launches"]
    count, ops.FLOP_COUNTER = ops.FLOP_COUNTER, {}
    try:
        out = _pipe(p).enable_request_adapter_scales()(**kw).images
        assert ops.FLOP_COUNTER.get("lora_expand", 0.0) == 0.0          # what ops._count saw of the expand launch
    finally:
        ops.FLOP_COUNTER = count
    assert ops.LORA_ROWS_COUNTER["launches"] == before
    assert torch.equal(out, ref)


def test_switch_off_refuses_differing_values(pair):
    p, reqs = pair, _Requests(R=2)
    for name in ("ipa_scale", "s_lora_scale", "c_lora_scale"):
        kw = _call_kw(reqs, (TRIPLES[0], TRIPLES[0]))
        kw[name] = [0.1, 0.7]
        with pytest.raises(ValueError, match=name):
            _pipe(p)(**kw)
        with pytest.raises(ValueError, match=name):
            _pipe(p).enable_request_adapter_scales().disable_request_adapter_scales()(**kw)
        kw[name] = [0.1, 0.7, 0.3]          # switch on: a length that is neither 1 nor R names the argument
        with pytest.raises(ValueError, match=name):
            _pipe(p).enable_request_adapter_scales()(**kw)


@torch.no_grad()
def test_equal_values_forced_down_the_row_route(pair):
    """the unfolded arithmetic alone: equal scales, but every argument handed to the processors as rows"""
    from imagdressing_amd import ops
    from imagdressing_amd.dressing_sd.pipelines._base import per_request_floats
    p, reqs = pair, _Requests(R=2)
    pipe = _pipe(p).enable_request_adapter_scales()
    pipe._adapter_scales = lambda name, value, R, neutral: (neutral, per_request_floats(name, value, R))
    before = ops.LORA_ROWS_COUNTER["launches"]
    out = pipe(**_call_kw(reqs, (TRIPLES[0], TRIPLES[0]))).images
    assert ops.LORA_ROWS_COUNTER["launches"] > before
    for r in range(2):
        st = _check(out[r:r + 1], _oracle(p, reqs, r, TRIPLES[0]), _traj_bar(p["dtype"]), floor=1.0)
        print(f"rows forced, request {r} [{p['dtype']}]: {st}")


@torch.no_grad()
def test_step_graph_replay_of_a_mixed_call_is_bit_identical(pair):
    from imagdressing_amd import scheduler as S
    p, reqs = pair, _Requests(R=2)
    kw = _call_kw(reqs, TRIPLES)
    eager = _pipe(p, S.DPMSolverMultistepScheduler(**KW)).enable_request_adapter_scales()(**kw).images
    pipe = _pipe(p, S.DPMSolverMultistepScheduler(**KW)).enable_request_adapter_scales().enable_step_graph()
    try:
        out = pipe(**kw).images
        assert pipe.__dict__.get("_last_step_graph") is not None          # the call did replay a captured step
    finally:
        pipe.release_step_graph()
    assert torch.equal(out, eager)


@torch.no_grad()
def test_deepcache_with_mixed_scales_matches_the_oracle_per_request(pair):
    p, reqs = pair, _Requests(R=2)
    pipe = _pipe(p).enable_request_adapter_scales().enable_deepcache(2, 1)
    out = pipe(**_call_kw(reqs, TRIPLES)).images
    from tests.test_deepcache_gpu import _check_traj
    for r in range(2):
        _check_traj(out[r:r + 1], _oracle(p, reqs, r, TRIPLES[r], deepcache=(2, 1)), p["dtype"], f"deepcache_adapter_scales_request{r}")
