"""Per-request ControlNet scale and guidance window on the host, without a GPU: the switch, the validation of the three arguments, the
route rule (equal triples -> the folded call, differing -> the table), the table itself (a hand-written case, two images per request,
the uncond half, PNDM's extra call), which ControlNet call every site of the loop makes, ``check_request``, the bookkeeping of
``SessionPlan`` / ``DenoiseSession`` on stand-ins, the properties of the CPU expression the GPU tests compare with, and that the
zero-conv dispatch does not look at ``out_scale``."""
import importlib
import inspect

import pytest
import torch

from imagdressing_amd import ops
from imagdressing_amd.dressing_sd.pipelines._base import (CONTROL_KEYS, PER_CALL_KEYS, PipelineBase, RequestLayout, control_plan,
                                                          control_request_values, control_scale_table, controlnet_keep, request_count)
from imagdressing_amd.session import SessionPlan, check_request
from tests import control_rows_cases as CC
from tests.test_deepcache_host import _RecordingUNet, _pipe
from tests.test_guidance_rescale_host import _SessionPipe, _SessionUNet

MODULES = ("IMAGDressing_v1_pipeline", "IMAGDressing_v1_pipeline_controlnet", "IMAGDressing_v1_pipeline_controlnet_inpainting",
           "IMAGDressing_v1_pipeline_ipa_controlnet")


# ---- the switch and the arguments ----
def test_every_pipeline_has_the_switch_off_by_default():
    for mod in MODULES:
        cls = importlib.import_module("imagdressing_amd.dressing_sd.pipelines." + mod).IMAGDressing_v1
        assert callable(cls.enable_request_control_scales) and callable(cls.disable_request_control_scales)
    pipe = PipelineBase()
    assert getattr(pipe, "_request_control_scales", False) is False
    assert pipe.enable_request_control_scales() is pipe and pipe._request_control_scales is True
    assert pipe.enable_request_control_scales(False) is pipe and pipe._request_control_scales is False
    assert pipe.enable_request_control_scales().disable_request_control_scales() is pipe and pipe._request_control_scales is False
    sig = inspect.signature(importlib.import_module("imagdressing_amd.dressing_sd.pipelines." + MODULES[1]).IMAGDressing_v1.open_session)
    assert sig.parameters["control_rows"].default is None


ARGS = dict(prompt=["a", "b", "c"], guidance_scale=7.5)
CTL = dict(controlnet_conditioning_scale=[1.0, 0.5, 0.8], control_guidance_start=[0.0, 0.2, 0.0], control_guidance_end=[1.0, 1.0, 0.5])


def _count(pipe, control, **per_call):
    per_call = dict(dict(num_inference_steps=10, eta=0.0, controlnet_conditioning_scale=control["controlnet_conditioning_scale"]), **per_call)
    return pipe._request_count(dict(ARGS), per_call, False, control=control)


def test_switch_off_a_differing_list_raises_as_before():
    assert "controlnet_conditioning_scale" in PER_CALL_KEYS
    pipe = _pipe(_RecordingUNet())
    with pytest.raises(ValueError, match="controlnet_conditioning_scale is per call"):
        _count(pipe, CTL)
    assert _count(pipe, dict(CTL, controlnet_conditioning_scale=[0.8, 0.8, 0.8])) == 3          # equal entries pass, as ever
    # ... and the window is not looked at: a list is read by its first entry
    assert control_plan(0.7, [0.3, 0.0], [0.9, 1.0], 2, 10) == (0.7, controlnet_keep(10, 0.3, 0.9), None)
    assert control_plan([0.7, 0.7], 0.0, 1.0, 2, 4, per_request=False) == (0.7, [1.0] * 4, None)


def test_switch_on_lists_are_accepted_and_checked_by_name():
    pipe = _pipe(_RecordingUNet()).enable_request_control_scales()
    assert _count(pipe, CTL) == 3
    assert _count(pipe, dict(CTL, control_guidance_end=1.0)) == 3 and _count(pipe, dict(CTL, controlnet_conditioning_scale=[0.4])) == 3
    for key in CONTROL_KEYS:
        with pytest.raises(ValueError, match=f"{key} has 2 entries for 3 requests"):
            _count(pipe, dict(CTL, **{key: CTL[key][:2]}))
    with pytest.raises(ValueError, match="num_inference_steps is per call"):          # the other per-call arguments stay per call
        _count(pipe, CTL, num_inference_steps=[10, 12, 10])
    for start, end in (([0.0, 0.5, 0.0], [1.0, 0.5, 1.0]), ([0.0, 0.6, 0.0], [1.0, 0.4, 1.0]), ([-0.1, 0.0, 0.0], 1.0), (0.0, [1.0, 1.1, 1.0]),
                       ([0.0, float("nan"), 0.0], 1.0)):
        with pytest.raises(ValueError, match=r"need 0 <= start < end <= 1"):
            _count(pipe, dict(CTL, control_guidance_start=start, control_guidance_end=end))
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="controlnet_conditioning_scale of request 1 must be finite"):
            _count(pipe, dict(CTL, controlnet_conditioning_scale=[1.0, bad, 0.8]))
    assert _count(pipe, dict(CTL, controlnet_conditioning_scale=[0.0, -1.0, 2.5])) == 3          # 0 and negative values are scales
    # the free function: the same with control=, and untouched without it
    assert request_count(dict(ARGS), dict(num_inference_steps=10), control=CTL) == 3
    assert control_request_values(**{k: v for k, v in zip(("scale", "start", "end"), CTL.values())}, R=3) == list(CC.ROUTE_TRIPLES)
    pipe.disable_request_control_scales()
    with pytest.raises(ValueError, match="controlnet_conditioning_scale is per call"):
        _count(pipe, CTL)


# ---- the route and the table ----
def test_equal_triples_give_no_table():
    for scale, start, end in ((0.8, 0.0, 1.0), ([0.8, 0.8, 0.8], 0.0, 1.0), ([0.8] * 3, [0.1] * 3, [0.9, 0.9, 0.9]), ([0.8], [0.1], 0.9)):
        s, keep, rows = control_plan(scale, start, end, 3, 10, per_request=True)
        first = lambda v: v[0] if isinstance(v, list) else v
        assert rows is None and s == 0.8 and keep == controlnet_keep(10, first(start), first(end))
    assert control_plan(0.8, 0.0, 1.0, 1, 5, per_request=True) == (0.8, [1.0] * 5, None)


def test_differing_triples_give_the_hand_written_table():
    scale, start, end = (list(v) for v in zip(*CC.ROUTE_TRIPLES))
    s, keep, rows = control_plan(scale, start, end, 3, CC.ROUTE_STEPS, per_request=True)
    assert s == 1.0 and keep == [1.0] * 10                               # the zero convs run at out_scale 1
    assert rows == [list(r) for r in CC.ROUTE_ROWS]
    # a difference in ANY of the three chooses the rows route
    assert control_plan(0.8, [0.0, 0.1], 1.0, 2, 10, per_request=True)[2] == [[0.8] * 10, [0.0] + [0.8] * 9]
    assert control_plan(0.8, 0.0, [1.0, 0.9], 2, 10, per_request=True)[2] == [[0.8] * 10, [0.8] * 9 + [0.0]]
    # one image per request: [calls, 2R], the uncond half repeats the cond half
    lay = RequestLayout(3, 1)
    tab = control_scale_table(rows, 10, lay, clamp=False)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (10, 6)
    for i in range(10):
        want = [CC.ROUTE_ROWS[r][i] for r in range(3)]
        assert tab[i].tolist() == [pytest.approx(v) for v in want + want]
    assert torch.equal(tab[:, :3], tab[:, 3:])
    # num_images_per_prompt = 2: request-major
    tab2 = control_scale_table(rows, 10, RequestLayout(3, 2), clamp=False)
    assert tuple(tab2.shape) == (10, 12)
    assert torch.equal(tab2[:, :6], tab[:, :3].repeat_interleave(2, dim=1)) and torch.equal(tab2[:, 6:], tab2[:, :6])
    assert tab2[3].tolist() == [pytest.approx(v) for v in [1.0, 1.0, 0.5, 0.5, 0.8, 0.8] * 2]
    # PNDM: one UNet call more than steps; the extra index keeps the last gate.  Without clamp a missing entry is an error
    tab3 = control_scale_table(rows, 11, lay, clamp=True)
    assert tuple(tab3.shape) == (11, 6) and torch.equal(tab3[:10], tab) and torch.equal(tab3[10], tab[9])
    with pytest.raises(ValueError, match="10 entries for 11 UNet calls"):
        control_scale_table(rows, 11, lay, clamp=False)


class _RecordingControlNet:
    """stand-in for the engine ControlNet: records the scalar and the row scales of every forward"""
    dtype = torch.float16

    def __init__(self):
        self.calls = []

    def forward_nhwc(self, x, t, ehs, cond, conditioning_scale=1.0, deepcache=None, scale_rows=None):
        self.calls.append(dict(scale=conditioning_scale, rows=None if scale_rows is None else scale_rows.clone(), rows_id=id(scale_rows),
                               cache=deepcache, batch=x.shape[0]))
        return [], None


@pytest.fixture
def no_launches(monkeypatch):
    for name in ("ddim_cfg_step", "sampler_step", "unipc_step"):
        monkeypatch.setattr(ops, name, lambda *a, **k: None)
    monkeypatch.setattr(ops, "lincomb", lambda terms, out=None: out if out is not None else terms[0][1].clone())
    monkeypatch.setattr(ops, "workspace", lambda tag, shape, dtype, device, init=None: torch.zeros(tuple(shape), dtype=dtype))


def _denoise(pipe, R, n, control, steps=10, **kw):
    pose = torch.zeros(1, 32, 32, 8, dtype=torch.float16)
    ctl = dict(image=pose, prompt_embeds=torch.zeros(R, 3, 8), negative_prompt_embeds=torch.zeros(R, 3, 8), **control)
    return pipe._denoise(latents=torch.zeros(R * n, 4, 4, 4), prompt_embeds=torch.zeros(R, 3, 8), negative_prompt_embeds=torch.zeros(R, 3, 8),
                         sa_hidden_states={}, num_inference_steps=steps, guidance_scale=7.5, requests=R, control=ctl, **kw)


@pytest.mark.parametrize("sched", ["ddim", "dpm", "pndm", "unipc", "unipc_fused"])
def test_every_call_site_of_the_loop_takes_the_route_of_the_call(no_launches, sched):
    pipe = _pipe(_RecordingUNet(), sched.split("_")[0])
    if sched == "unipc_fused":
        pipe.scheduler.enable_fused_step()
    cn = pipe.controlnet = _RecordingControlNet()
    calls = 11 if sched == "pndm" else 10
    # folded: the scalar times the gate of the step, no rows -- the call the parent makes
    s, keep, rows = control_plan([0.8, 0.8, 0.8], 0.2, 1.0, 3, 10, per_request=True)
    _denoise(pipe, 3, 1, dict(scale=s, keep=keep, rows=rows))
    assert len(cn.calls) == calls and all(c["rows"] is None for c in cn.calls)
    assert [c["scale"] for c in cn.calls] == [0.0, 0.0] + [0.8] * (calls - 2)
    cn.calls.clear()
    _denoise(pipe, 3, 1, dict(scale=0.8, keep=keep))                         # (a control dict without the key: as before)
    assert [c["scale"] for c in cn.calls] == [0.0, 0.0] + [0.8] * (calls - 2) and all(c["rows"] is None for c in cn.calls)
    cn.calls.clear()
    # rows: out_scale 1 and row i of the table at UNet call i, PNDM's extra call on the last gate
    scale, start, end = (list(v) for v in zip(*CC.ROUTE_TRIPLES))
    s, keep, rows = control_plan(scale, start, end, 3, 10, per_request=True)
    _denoise(pipe, 3, 2, dict(scale=s, keep=keep, rows=rows))
    assert len(cn.calls) == calls and all(c["scale"] == 1.0 and c["batch"] == 12 for c in cn.calls)
    for i, c in enumerate(cn.calls):
        want = [CC.ROUTE_ROWS[r][min(i, 9)] for r in range(3) for _ in range(2)]
        assert c["rows"].dtype == torch.float32 and c["rows"].tolist() == [pytest.approx(v) for v in want + want]
    with pytest.raises(ValueError, match="2 requests' scales for 3 requests"):
        _denoise(pipe, 3, 1, dict(scale=1.0, keep=keep, rows=rows[:2]))


def test_rows_route_composes_with_deepcache(no_launches):
    pipe = _pipe(_RecordingUNet(), "ddim").enable_deepcache(cache_interval=2, depth=1)
    cn = pipe.controlnet = _RecordingControlNet()
    _denoise(pipe, 2, 1, dict(scale=1.0, keep=[1.0] * 4, rows=[[1.0] * 4, [0.5, 0.5, 0.0, 0.0]]), steps=4)
    assert all(c["cache"] is not None and c["rows"] is not None for c in cn.calls)          # the cache keyword and the rows, on every call
    assert len({id(c["cache"]) for c in cn.calls}) == 1 and cn.calls[0]["cache"] is pipe.unet.calls[0]["cache"]
    assert [c["rows"].tolist() for c in cn.calls] == [[1.0, 0.5] * 2, [1.0, 0.5] * 2, [1.0, 0.0] * 2, [1.0, 0.0] * 2]


# ---- the ControlNet engine's argument checks (no launch is reached) ----
def test_controlnet_refuses_both_a_scalar_and_rows():
    from imagdressing_amd.unet import ControlNetModel
    cn = object.__new__(ControlNetModel)
    x = torch.zeros(4, 2, 2, 8, dtype=torch.float16)
    with pytest.raises(ValueError, match="scale_rows and conditioning_scale = 0.5 were both given"):
        cn.forward_nhwc(x, 0, None, None, 0.5, scale_rows=torch.ones(4))
    with pytest.raises(ValueError, match="scale_rows must be a 1-d fp32 device tensor of 4 values"):
        cn.forward_nhwc(x, 0, None, None, 1.0, scale_rows=torch.ones(2))
    sig = inspect.signature(ControlNetModel.forward_nhwc)
    assert sig.parameters["conditioning_scale"].default == 1.0 and sig.parameters["scale_rows"].default is None


# ---- sessions ----
def test_check_request_keeps_its_refusal_without_control_rows_and_lifts_it_with():
    ok = dict(size=(128, 128), num_inference_steps=4, guidance_scale=7.5)
    assert inspect.signature(check_request).parameters["control_rows"].default is False
    for kw in (dict(control_guidance_start=0.2), dict(control_guidance_end=0.8)):
        with pytest.raises(NotImplementedError, match="control_guidance_start / control_guidance_end"):
            check_request(**ok, **kw)
        with pytest.raises(NotImplementedError, match="control_guidance_start / control_guidance_end"):
            check_request(control_rows=False, **ok, **kw)
        check_request(control_rows=True, **ok, **kw)
    with pytest.raises(NotImplementedError, match="opened without control_rows"):
        check_request(controlnet_conditioning_scale=0.5, **ok)
    check_request(control_rows=True, controlnet_conditioning_scale=0.5, control_guidance_start=0.25, control_guidance_end=0.75, **ok)
    check_request(control_rows=True, controlnet_conditioning_scale=None, **ok)
    check_request(control_rows=True, controlnet_conditioning_scale=-1.0, **ok)
    for a, b in ((0.5, 0.5), (0.6, 0.4), (-0.1, 1.0), (0.0, 1.5), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="need 0 <= start < end <= 1"):
            check_request(control_rows=True, control_guidance_start=a, control_guidance_end=b, **ok)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="controlnet_conditioning_scale must be finite"):
            check_request(control_rows=True, controlnet_conditioning_scale=bad, **ok)
    with pytest.raises(ValueError, match="controlnet_conditioning_scale is per request in a session"):
        check_request(control_rows=True, controlnet_conditioning_scale=[0.5, 0.6], **ok)


def _sched(name="dpm"):
    return _pipe(_RecordingUNet(), name).scheduler


def test_session_plan_carries_each_runs_effective_scale():
    plan = SessionPlan(3, _sched(), control_rows=True, control_scale=0.9)
    a = plan.submit(4, control=(0.6, 0.0, 0.5))
    b = plan.submit(2)                                                       # names nothing: the plan's scale, the whole schedule
    assert a.control == [pytest.approx(0.6)] * 2 + [0.0, 0.0] and b.control == [0.9, 0.9]
    plan.admit()
    st = plan.next_rows()
    assert st.control_rows == [pytest.approx(v) for v in [0.6, 0.9, 1.0] * 2]          # [cond; uncond], the idle slot at 1.0
    c = plan.submit(5, control=(None, 0.4, 1.0))                              # admitted at another step, into slot 2
    plan.admit()
    assert plan.next_rows().control_rows == [pytest.approx(v) for v in [0.6, 0.9, 0.0] * 2]          # b's last step; c: 0/5 < 0.4 closed
    assert plan.next_rows().control_rows == [pytest.approx(v) for v in [0.0, 1.0, 0.0] * 2]          # a past its window; slot 1 idle again
    assert plan.next_rows().control_rows == [pytest.approx(v) for v in [0.0, 1.0, 0.9] * 2]          # a's last step; c: 2/5 >= 0.4 open
    assert plan.next_rows().control_rows == [pytest.approx(v) for v in [1.0, 1.0, 0.9] * 2]
    assert c.control == [0.0, 0.0, 0.9, 0.9, 0.9]
    # without the flag: no rows, and a run that names a gate is refused
    plain = SessionPlan(2, _sched())
    plain.submit(3)
    plain.admit()
    assert plain.next_rows().control_rows is None
    with pytest.raises(NotImplementedError, match="without control_rows"):
        plain.submit(3, control=(0.5, 0.0, 1.0))


def test_session_plan_pndm_extra_call_keeps_the_last_gate():
    plan = SessionPlan(1, _sched("pndm"), control_rows=True)
    run = plan.submit(4, control=(0.5, 0.0, 0.75))
    assert run.steps == 5 and run.control == [0.5, 0.5, 0.5, 0.0, 0.0]


def test_compacting_plan_writes_the_scales_by_row():
    plan = SessionPlan(3, _sched(), compact=True, control_rows=True)
    a, b, c = plan.submit(1, control=(0.3, 0.0, 1.0)), plan.submit(3, control=(0.6, 0.0, 1.0)), plan.submit(3, control=(0.7, 0.0, 1.0))
    plan.admit()
    st = plan.next_rows()
    assert st.width == 3 and st.control_rows == [pytest.approx(v) for v in [0.3, 0.6, 0.7] * 2]
    st = plan.next_rows()                                                    # a left: width 2, a repack -- slots 1 and 2 now sit in rows 0 and 1
    assert st.width == 2 and st.repack and st.row_slot == [1, 2]
    assert st.control_rows == [pytest.approx(v) for v in [0.6, 0.7] * 2]


class _SessionControlNet(_SessionUNet):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward_nhwc(self, x, t, ehs, cond, conditioning_scale=1.0, deepcache=None, scale_rows=None):
        self.calls.append(dict(scale=conditioning_scale, rows=None if scale_rows is None else scale_rows.clone(), rows_id=id(scale_rows),
                               batch=x.shape[0]))
        return [], None


@pytest.fixture
def session_stand_ins(monkeypatch):
    for name in ("sampler_step_rows", "sampler_step_rows_at", "session_input_rows"):
        monkeypatch.setattr(ops, name, lambda *a, **k: None)
    monkeypatch.setattr(ops, "ensure_device", lambda device: None)


def _session_pipe():
    pipe = _SessionPipe()
    pipe._init_common(vae=None, reference_unet=None, unet=_SessionUNet(), tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None,
                      scheduler=_sched(), controlnet=_SessionControlNet())
    return pipe


def _submit(ses, steps, **kw):
    return ses.submit(num_inference_steps=steps, guidance_scale=7.5, prompt_embeds=torch.zeros(1, 3, 8), negative_prompt_embeds=torch.zeros(1, 3, 8),
                      latents=torch.zeros(1, 4, 4, 4), pose_image=torch.zeros(1, 3, 32, 32), output_type="latent", **kw)


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
def test_a_control_rows_session_always_takes_the_rows_route(session_stand_ins, compact):
    pipe = _session_pipe()
    cn = pipe.controlnet
    with pipe._open_session(3, 32, 32, 0.9, with_controlnet=True, compact=compact, control_rows=True) as ses:
        assert ses.control_rows and ses.control_scale_rows.tolist() == [1.0] * 6
        a = _submit(ses, 4, controlnet_conditioning_scale=0.6, control_guidance_end=0.5)
        b = _submit(ses, 2)                                                  # the session's 0.9, equal company or not: still the rows route
        ses.step()
        B = ses.width
        assert B == (2 if compact else 3) and cn.calls[0]["scale"] == 1.0 and cn.calls[0]["batch"] == 2 * B
        assert cn.calls[0]["rows"].tolist() == [pytest.approx(v) for v in ([0.6, 0.9] if compact else [0.6, 0.9, 1.0]) * 2]
        ses.drain()
        assert a.done and b.done and len(cn.calls) == 4 and all(c["scale"] == 1.0 and c["rows"] is not None for c in cn.calls)
        assert cn.calls[3]["rows"][0] == 0.0                                 # a's last step lies past its window
        if not compact:
            assert len({c["rows_id"] for c in cn.calls}) == 1                  # one view object per width: a fixed address
    with pipe._open_session(2, 32, 32, 0.9, with_controlnet=True, compact=compact, control_rows=True) as ses:
        _submit(ses, 2), _submit(ses, 2)                                      # all at the session's value: the rows route all the same
        cn.calls.clear()
        ses.drain()
        assert [c["rows"].tolist() for c in cn.calls] == [[pytest.approx(0.9)] * 4] * 2 and all(c["scale"] == 1.0 for c in cn.calls)


def test_a_default_session_issues_the_parents_call_and_keeps_the_refusal(session_stand_ins):
    pipe = _session_pipe()
    cn = pipe.controlnet
    with pipe._open_session(2, 32, 32, 0.9, with_controlnet=True) as ses:
        assert not ses.control_rows and ses.control_scale_rows is None
        with pytest.raises(NotImplementedError, match="control_guidance_start / control_guidance_end"):
            _submit(ses, 2, control_guidance_end=0.5)
        with pytest.raises(NotImplementedError, match="opened without control_rows"):
            _submit(ses, 2, controlnet_conditioning_scale=0.5)
        _submit(ses, 2)
        ses.drain()
        assert [(c["scale"], c["rows"]) for c in cn.calls] == [(0.9, None)] * 2
    # control_rows=None follows the pipeline switch as it stands when the session opens; an explicit False wins over it
    pipe.enable_request_control_scales()
    with pipe._open_session(2, 32, 32, 0.9, with_controlnet=True) as ses:
        assert ses.control_rows
    with pipe._open_session(2, 32, 32, 0.9, with_controlnet=True, control_rows=False) as ses:
        assert not ses.control_rows
    with pipe._open_session(2, 32, 32) as ses:                                # a session without a ControlNet has nothing to scale
        assert not ses.control_rows
    with pytest.raises(ValueError, match="control_rows needs a ControlNet"):
        pipe._open_session(2, 32, 32, control_rows=True)


# ---- the expression the GPU bars rest on ----
@pytest.mark.parametrize("name,dt", CC.DTYPES)
def test_the_oracle_expression_has_the_stated_double_rounding_properties(name, dt):
    """rows route RNE16(s RNE16(y)) against folded RNE16(s y), y = W x + b in fp32: at most one unit in the last place, about a
    quarter of the elements differ, none for a power of two in bf16, in fp16 none outside the subnormal products"""
    g = torch.Generator().manual_seed(5)
    y = torch.randn(1 << 20, generator=g)                                     # the fp32 sum of a zero conv
    for s in (0.05, 0.3, 0.8, 1.3, 1.999):
        sf = torch.tensor(s, dtype=torch.float32)
        folded, rows = (y * sf).to(dt), CC.oracle(y.to(dt), s)
        d = CC.ulp_distance(folded, rows)
        assert int(d.max()) == 1, (s, int(d.max()))
        assert 0.05 < float((d > 0).float().mean()) < 0.45, (s, float((d > 0).float().mean()))
    tiny = torch.finfo(dt).tiny
    for s in (0.5, 0.25, 2.0, 2.0 ** -10):
        sf = torch.tensor(s, dtype=torch.float32)
        folded, rows = (y * sf).to(dt), CC.oracle(y.to(dt), s)
        differ = CC.bits(folded) != CC.bits(rows)
        if dt is torch.bfloat16:
            assert not differ.any(), s
        else:          # fp16: exact unless the scaled value (or the value itself) is subnormal, where the spacing no longer halves
            normal = ((y * sf).abs() >= tiny) & (y.abs() >= tiny)
            assert not (differ & normal).any(), s
            assert int(CC.ulp_distance(folded, rows).max()) <= 1
    assert torch.equal(CC.oracle(y.to(dt), 1.0), y.to(dt))                     # s = 1 is the identity on 16-bit data


def test_expected_leaves_rows_at_one_alone_nan_payloads_included():
    x = torch.tensor([[0x7FC1, 0x7E01, 0x3C00, 0x0001], [0x7FC1, 0x7E01, 0x3C00, 0x0001]], dtype=torch.int32).to(torch.int16).view(torch.float16)
    out = CC.expected(x, [1.0, 2.0])
    assert torch.equal(CC.bits(out[0]), CC.bits(x[0]))
    assert float(out[1, 2]) == 2.0 and out[1, 3].view(torch.int16).item() == 2


# ---- the zero-conv dispatch does not depend on out_scale ----
def test_zero_conv_dispatch_does_not_look_at_out_scale():
    """the engine test compares a forward at out_scale = s with one at out_scale = 1 followed by the row scale: both must go through the
    same tile configuration, K split and entry point, for every residual shape at the tested latents"""
    import os
    from imagdressing_amd import _lib
    from tests import dispatch_recorder as DR
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    shapes = []
    for h, w, B in ((16, 16, 4), (8, 8, 4), (64, 80, 8)):
        pix, ch = h * w, (320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280, 1280)
        div = (1, 1, 1, 4, 4, 4, 16, 16, 16, 64, 64, 64, 64)
        shapes += [(B * max(pix // d, 1), c) for c, d in zip(ch, div)]
    with DR.harness(ops, _lib.load()) as hs:
        for name, dt in DR.DTYPES:
            for M, C_ in sorted(set(shapes)):
                got = []
                for scale in (1.0, 0.8, 0.0):
                    ops._CFG_DECISIONS.clear()
                    hs.proxy.launches = []
                    ops.conv_gemm(torch.empty(M, C_, dtype=dt), torch.empty(C_, C_, dtype=dt), M=M, N=C_, Cin=C_, taps=1, Hin=1, Win=1, Hout=1, Wout=1,
                                  bias=torch.empty(C_), out_scale=scale)
                    got.append(hs.proxy.launches)
                assert got[0] == got[1] == got[2] and len(got[0]) == 1, (name, M, C_, got)
