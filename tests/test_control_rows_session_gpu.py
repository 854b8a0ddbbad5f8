"""Per-request ControlNet scale and guidance window in denoising sessions (``open_session(control_rows=True)``) on the GPU: SMALL config
with a ControlNet, 3 slots at 128 x 128, DPM-Solver++ and DDIM, 6 to 8 steps.  A request's final latent is the same bit for bit
whatever runs in the other slots (a ``control_rows`` session always takes the rows route), plain and compacting at a fixed width; a
staggered pair follows the gated oracle at each request's own values; a default session refuses a window and keeps the parent's bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair  # noqa: E402
from tests.test_control_rows_pipeline_gpu import GS, MIXED, STEPS, _dpm, _oracle, _pose  # noqa: E402
from tests.test_multi_request_gpu import _check, _Requests, _sched, _traj_bar  # noqa: E402
from tests.test_session_gpu import _submit_kw  # noqa: E402


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def setup(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    dt = request.param
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dt)
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    return dict(p=p, pipe=pipe, dtype=dt, reqs=_Requests(R=3), pose=_pose() + [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(18))])


def _kw(s, r, steps, **over):
    return _submit_kw(s["reqs"], r, steps, guidance=GS + (6.0,), image_scale=(1.0, 1.0, 1.0), pose_image=s["pose"][r].cuda(), **over)


A = dict(controlnet_conditioning_scale=0.6, control_guidance_start=0.0, control_guidance_end=0.5)


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
@pytest.mark.parametrize("name", ["dpm", "ddim"])
@torch.no_grad()
def test_a_request_does_not_see_its_companys_scales_or_windows(setup, name, compact):
    """request A = (0.6, 0, 0.5), 8 steps, slot 0: alone, then with requests of other scales, windows and step counts admitted at steps 2
    and 4.  Compacting at the fixed width ladder (3,): the batch stays 3 rows wide, so no tile choice moves either."""
    from imagdressing_amd import ops
    pipe = setup["pipe"]
    pipe.scheduler = _sched() if name == "ddim" else _dpm()
    kw = dict(compact=True, widths=(3,)) if compact else {}
    try:
        with pipe.open_session(slots=3, width=128, height=128, control_rows=True, **kw) as ses:
            a = ses.submit(**_kw(setup, 0, 8, **A))
            before = ops.SCALE_ROWS_COUNTER["launches"]
            ses.drain()
            assert ops.SCALE_ROWS_COUNTER["launches"] == before + 8             # one launch per step, idle company or not
            alone = a.result().images
        with pipe.open_session(slots=3, width=128, height=128, control_rows=True, **kw) as ses:
            a = ses.submit(**_kw(setup, 0, 8, **A))
            ses.step(), ses.step()
            b = ses.submit(**_kw(setup, 1, 7, controlnet_conditioning_scale=1.3, control_guidance_start=0.3))
            ses.step(), ses.step()
            c = ses.submit(**_kw(setup, 2, 6, control_guidance_end=0.4))          # the session's scale (1.0), its own window
            ses.drain()
            assert (a.slot, b.slot, c.slot) == (0, 1, 2) and ses.steps_run == 10
            crowded = a.result().images
            assert torch.isfinite(b.result().images).all() and torch.isfinite(c.result().images).all()
    finally:
        pipe.scheduler = _sched()
    assert torch.isfinite(alone).all()
    assert torch.equal(alone, crowded), (alone - crowded).abs().max().item()


@torch.no_grad()
def test_the_window_and_the_scale_reach_the_request(setup):
    """sensitivity: the same request with another window, and with another scale, ends elsewhere"""
    pipe, outs = setup["pipe"], []
    for ctl in (A, dict(A, control_guidance_end=1.0), dict(A, controlnet_conditioning_scale=0.3)):
        with pipe.open_session(slots=3, width=128, height=128, control_rows=True) as ses:
            t = ses.submit(**_kw(setup, 0, 6, **ctl))
            ses.drain()
            outs.append(t.result().images)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    for o in outs[1:]:
        rel = ((o - outs[0]).pow(2).mean().sqrt() / outs[0].pow(2).mean().sqrt()).item()
        print(f"control_rows session sensitivity {setup['dtype']}: rel rms {rel:.4e}")
        assert rel > 1e-3


@torch.no_grad()
def test_staggered_requests_follow_the_gated_oracle(setup):
    """two requests of 8 steps (the step count ``_traj_bar`` was set on), the second admitted after step 2, each with its own scale and
    window: against the reference loop at batch 1 driving the gated oracle ControlNet at that request's values"""
    p, pipe, dt = setup["p"], setup["pipe"], setup["dtype"]
    with pipe.open_session(slots=3, width=128, height=128, controlnet_conditioning_scale=0.8, control_rows=True) as ses:
        a = ses.submit(**_kw(setup, 0, STEPS))                                # names nothing: the session's 0.8 over the whole schedule
        ses.step(), ses.step()
        b = ses.submit(**_kw(setup, 1, STEPS, controlnet_conditioning_scale=MIXED["controlnet_conditioning_scale"][1],
                             control_guidance_start=MIXED["control_guidance_start"][1], control_guidance_end=MIXED["control_guidance_end"][1]))
        ses.drain()
        assert (a.slot, b.slot) == (0, 1) and ses.steps_run == STEPS + 2
    for r, t in enumerate((a, b)):
        triple = tuple(MIXED[k][r] for k in MIXED)
        st = _check(t.result().images, _oracle(p, setup["reqs"], r, *triple), _traj_bar(dt), floor=1.0)
        print(f"control_rows session request {r} {triple} [{dt}]: {st}")


@torch.no_grad()
def test_a_default_session_refuses_a_window_and_keeps_the_parents_bits(setup):
    from imagdressing_amd import ops
    pipe, outs = setup["pipe"], []
    before = ops.SCALE_ROWS_COUNTER["launches"]
    for on, kw in ((False, {}), (True, dict(control_rows=False))):
        pipe.enable_request_control_scales(on)
        try:
            with pipe.open_session(slots=3, width=128, height=128, controlnet_conditioning_scale=0.8, **kw) as ses:
                assert not ses.control_rows
                with pytest.raises(NotImplementedError, match="control_guidance"):
                    ses.submit(**_kw(setup, 0, 6, control_guidance_end=0.5))
                with pytest.raises(NotImplementedError, match="without control_rows"):
                    ses.submit(**_kw(setup, 0, 6, controlnet_conditioning_scale=0.5))
                t = ses.submit(**_kw(setup, 0, 6))
                ses.drain()
                outs.append(t.result().images)
        finally:
            pipe.disable_request_control_scales()
    assert ops.SCALE_ROWS_COUNTER["launches"] == before                      # neither session launched the row scale
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    pipe.enable_request_control_scales()
    try:          # control_rows=None follows the switch: the rows route, and at 0.8 not the folded bits
        with pipe.open_session(slots=3, width=128, height=128, controlnet_conditioning_scale=0.8) as ses:
            assert ses.control_rows
            t = ses.submit(**_kw(setup, 0, 6))
            ses.drain()
    finally:
        pipe.disable_request_control_scales()
    assert ops.SCALE_ROWS_COUNTER["launches"] == before + 6
    st = _check(t.result().images, outs[0], _traj_bar(setup["dtype"]), floor=1.0)          # one more rounding of the residuals: close, within the path's bar
    print(f"control_rows session rows route against the folded session [{setup['dtype']}]: {st}")
