"""Compacting denoising sessions on the GPU (``pipe.open_session(..., compact=True, widths=...)``): every step runs a batch as wide as
the running requests need.  At full width and alone the results equal the non-compacting session bit for bit; staggered, shrinking and
laddered traces against the reference loop at batch 1 within the bars of tests/test_session_gpu.py; which row every slot ran in; the
ControlNet pipeline; the life cycle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair  # noqa: E402
from tests.test_multi_request_gpu import _bar_small, _check, _Requests, _sched, _traj_bar  # noqa: E402
from tests.test_session_gpu import _engine_scheduler, _pipe, _reference, _submit_kw, small_pair  # noqa: E402,F401

SIZE = dict(width=128, height=128)


def _bars(name, dtype):
    """those of test_staggered_requests_match_the_reference_loop: DDIM the request-batched call's, the others the trajectory bars"""
    return (_bar_small(dtype), 0.0) if name == "ddim" else (_traj_bar(dtype), 1.0)


def _against_reference(p, reqs, name, tickets, what):
    for t, (r, steps) in tickets:
        out = t.result().images
        assert out.shape == (1, 4, 16, 16)
        bar, floor = _bars(name, p["dtype"])
        st = _check(out, _reference(p, reqs, name, r, steps), bar, floor=floor)
        print(f"{what} {name} request {r} ({steps} steps) [{p['dtype']}]: {st}")


def _staggered(pipe, reqs, steps=(12, 8, 10), slots=2, **open_kw):
    """the trace of test_staggered_requests_match_the_reference_loop -> (tickets, the session's counters)"""
    with pipe.open_session(slots=slots, **SIZE, **open_kw) as ses:
        a = ses.submit(**_submit_kw(reqs, 0, steps[0]))
        for _ in range(4):
            ses.step()
        b = ses.submit(**_submit_kw(reqs, 1, steps[1]))
        c = ses.submit(**_submit_kw(reqs, 2, steps[2]))
        ses.drain()
        stats = dict(steps_at_width=dict(ses.steps_at_width), repacks=ses.repacks, steps_run=ses.steps_run, slots=(a.slot, b.slot, c.slot))
    return (a, b, c), stats


# ---- bit for bit against the session that does not compact ----
@pytest.mark.parametrize("name", ["dpm", "ddim"])
@torch.no_grad()
def test_full_width_equals_the_default_session(small_pair, name):
    """widths=(3,) never repacks and runs what compact=False runs (rows and slots fall free together, so row == slot): the staggered
    three-request trace, and three requests admitted together, equal the default session for every request"""
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _engine_scheduler(name))
    plain, s0 = _staggered(pipe, reqs, slots=3)
    full, s1 = _staggered(pipe, reqs, slots=3, compact=True, widths=(3,))
    assert s0["steps_at_width"] == s1["steps_at_width"] == {3: 14} and s0["repacks"] == s1["repacks"] == 0 and s1["slots"] == (0, 1, 2)
    for r, (x, y) in enumerate(zip(plain, full)):
        assert torch.equal(x.result().images, y.result().images), (r, (x.result().images - y.result().images).abs().max().item())
    outs = []
    for kw in (dict(), dict(compact=True)):
        with pipe.open_session(slots=3, **SIZE, **kw) as ses:
            tickets = [ses.submit(**_submit_kw(reqs, r, 6)) for r in range(3)]
            assert ses.drain() == tickets and ses.steps_at_width == {3: 6} and ses.repacks == 0 and ses.width == 3 and ses.rows == [None] * 3
        outs.append([t.result().images for t in tickets])
    for r in range(3):
        assert torch.equal(outs[0][r], outs[1][r]), r


@pytest.mark.parametrize("name", ["dpm", "euler"])
@torch.no_grad()
def test_alone_equals_a_one_slot_session(small_pair, name):
    """one request in a compacting 3-slot session runs the launch list of a slots=1 session: bit for bit, at width 1 throughout (the
    first layout moves nothing: no repack)"""
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _engine_scheduler(name))
    n = 7
    with pipe.open_session(slots=1, **SIZE) as ses:
        t1 = ses.submit(**_submit_kw(reqs, 1, n))
        ses.drain()
        assert ses.steps_at_width == {1: n}
    with pipe.open_session(slots=3, **SIZE, compact=True) as ses:
        t3 = ses.submit(**_submit_kw(reqs, 1, n))
        ses.step()
        assert ses.width == 1 and ses.rows == [0] and t3.slot == 0
        ses.drain()
        assert ses.steps_at_width == {1: n} and ses.repacks == 0 and ses.steps_run == n
    assert torch.equal(t1.result().images, t3.result().images), (t1.result().images - t3.result().images).abs().max().item()


# ---- traces against the reference loop ----
@pytest.mark.parametrize("name", ["ddim", "dpm", "euler"])
@torch.no_grad()
def test_staggered_requests_match_the_reference_loop(small_pair, name):
    """12 / 8 / 10 steps on 2 slots: 4 steps at width 1, 8 at width 2 (repack 1 -> 2: the second request's input and the first one's,
    re-laid from its fp32 latent), then the queued third alone in slot 0 (repack 2 -> 1)"""
    p, reqs = small_pair, _Requests()
    (a, b, c), stats = _staggered(_pipe(p, _engine_scheduler(name)), reqs, compact=True)
    assert stats == dict(steps_at_width={1: 14, 2: 8}, repacks=2, steps_run=22, slots=(0, 1, 0))
    _against_reference(p, reqs, name, [(a, (0, 12)), (b, (1, 8)), (c, (2, 10))], "compact session")


def _shrink(pipe, reqs, order):
    """three requests submitted together on 3 slots, ``order`` = [(request, steps)] by slot -> tickets, rows after every step"""
    with pipe.open_session(slots=3, **SIZE, compact=True) as ses:
        tickets = [ses.submit(**_submit_kw(reqs, r, n)) for r, n in order]
        seen = []
        while ses.plan.running or ses.plan.pending:
            ses.step()
            seen.append((ses.width, ses.rows, ses.repacks))
        assert ses.steps_at_width == {3: 4, 2: 2, 1: 3}
    return tickets, seen


@torch.no_grad()
def test_shrink_with_a_mover(small_pair):
    """4 / 9 / 6 steps on 3 slots (DPM-Solver++: the history stays in the slot while the row moves): widths 3 -> 2 -> 1, the survivor
    moves from row 1 to row 0"""
    p, reqs = small_pair, _Requests()
    order = [(0, 4), (1, 9), (2, 6)]
    tickets, seen = _shrink(_pipe(p, _engine_scheduler("dpm")), reqs, order)
    assert [w for w, _, _ in seen] == [3, 3, 3, 3, 2, 2, 1, 1, 1] and [k for _, _, k in seen] == [0] * 4 + [1] * 2 + [2] * 3
    assert seen[2][1] == [0, 1, 2] and seen[3][1] == [None, 1, 2]          # (rows as the step left them: the finished request is gone)
    assert seen[4][1] == [1, 2] and seen[5][1] == [1, None] and seen[6][1] == [1] and seen[8][1] == [None]
    assert [t.slot for t in tickets] == [0, 1, 2]
    _against_reference(p, reqs, "dpm", list(zip(tickets, order)), "shrinking session")


def _slot_of_request_1(pipe, reqs, first):
    """request 1 (9 steps) in a default 3-slot session next to request 0 (9 steps): submitted first (slot 0) or second (slot 1)"""
    with pipe.open_session(slots=3, **SIZE) as ses:
        order = [1, 0] if first else [0, 1]
        t = {r: ses.submit(**_submit_kw(reqs, r, 9)) for r in order}
        ses.drain()
        assert t[1].slot == (0 if first else 1)
    return t[1].result().images


@torch.no_grad()
def test_position_independence(small_pair):
    """Prerequisite: in a default session the same request gets the same bits in slot 0 and in slot 1 (every launch on the path is
    row-local).  Then the 9-step request of the shrink trace gets the same latent whether it was submitted first (row 0 throughout)
    or second (row 1, then row 0): the width sequences are equal."""
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _engine_scheduler("dpm"))
    in0, in1 = _slot_of_request_1(pipe, reqs, True), _slot_of_request_1(pipe, reqs, False)
    assert torch.equal(in0, in1), (in0 - in1).abs().max().item()
    first, seen_f = _shrink(pipe, reqs, [(1, 9), (0, 4), (2, 6)])
    second, seen_s = _shrink(pipe, reqs, [(0, 4), (1, 9), (2, 6)])
    assert [w for w, _, _ in seen_f] == [w for w, _, _ in seen_s]
    assert seen_f[4][1] == [0, 2] and seen_f[6][1] == [0] and seen_s[4][1] == [1, 2] and seen_s[6][1] == [1]
    x, y = first[0].result().images, second[1].result().images
    assert torch.equal(x, y), (x - y).abs().max().item()


@torch.no_grad()
def test_ladder_keeps_an_idle_row(small_pair):
    """widths (1, 2, 4) on 4 slots: 3 running run at width 4 with one idle row; a fourth takes it; the departure 4 -> 3 does not
    repack and leaves row 1 idle; a later admission takes exactly that row.  Step counts 8 / 10 / 12 only, the ones ``_bar_small`` is
    used at elsewhere (a first version of this test ran request 1 for 3 steps: fp16 rel_rms 3.0e-3, bf16 2.4e-2 with max_abs 0.119 x std
    against the bar's 0.1 -- 8x the fp16 figure, the ratio of the two formats' precision, on a latent that is still mostly noise; a SOLO
    pipeline call of that request, no session involved, measured the same 2.4e-2 / 0.119 x std)."""
    p, reqs = small_pair, _Requests()
    name = "ddim"
    pipe = _pipe(p, _engine_scheduler(name))
    with pipe.open_session(slots=4, **SIZE, compact=True, widths=(1, 2, 4)) as ses:
        a, b, c = (ses.submit(**_submit_kw(reqs, r, n)) for r, n in ((0, 12), (1, 8), (2, 12)))
        ses.step()
        assert ses.width == 4 and ses.rows == [0, 1, 2, None] and ses.repacks == 0
        d = ses.submit(**_submit_kw(reqs, 0, 10))
        ses.step()
        assert ses.rows == [0, 1, 2, 3] and d.slot == 3
        for _ in range(5):
            assert ses.step() == []
        assert ses.step() == [b] and ses.rows == [0, None, 2, 3]
        ses.step()
        assert ses.width == 4 and ses.rows == [0, None, 2, 3] and ses.repacks == 0          # 3 running: no repack, the row idles
        e = ses.submit(**_submit_kw(reqs, 1, 8))
        ses.step()
        assert ses.rows == [0, 1, 2, 3] and e.slot == 1 and ses.repacks == 0
        ses.step()                                         # d leaves with step 11, a and c with step 12: 3 running, still width 4
        assert ses.step() == [a, c] and ses.width == 4 and ses.repacks == 0 and ses.rows == [None, 1, None, None]
        ses.step()                                         # e alone: 4 -> 1, the one repack of the trace
        assert ses.width == 1 and ses.rows == [1] and ses.repacks == 1
        ses.drain()
        assert ses.steps_at_width == {4: 12, 1: 5} and ses.repacks == 1 and ses.steps_run == 17
    _against_reference(p, reqs, name, [(a, (0, 12)), (b, (1, 8)), (c, (2, 12)), (d, (0, 10)), (e, (1, 8))], "laddered session")


_CTRL_REF = {}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@torch.no_grad()
def test_controlnet_compact_session_staggered(dtype):
    """the ControlNet (pose) pipeline, two staggered requests with their own pose images against the oracle with its ControlNet, 8 steps
    each (the count ``_traj_bar`` was set on: test_session_gpu.test_controlnet_session_staggered).  The second enters after two steps, so
    the first finishes two steps before it: the session runs widths 1, 1, 2 x 6, 1, 1 and the last two steps carry the survivor's pose
    image in row 0, re-laid by the repack."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    from oracle.ddim import DDIMOracle
    from oracle.pipeline import denoise
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=dtype)
    reqs, steps, gs = _Requests(R=2), (8, 8), (5.0, 7.0)
    pose = [torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(16 + r)) for r in range(2)]
    if not _CTRL_REF:          # (the fp32 CPU oracle is the same for both element types: computed once)
        for r in range(2):
            _CTRL_REF[r] = denoise(p["o_unet"], p["o_ref"], DDIMOracle(), reqs.latent(r), reqs.pe[r], reqs.ne[r], reqs.cloth[r], reqs.refl[r],
                                   steps[r], gs[r], controlnet=p["o_ctrl"], control_image=pose[r],
                                   prompt_embeds_control=torch.cat([reqs.ne[r], reqs.pe[r]]), conditioning_scale=0.8)
    pipe = IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           controlnet=p["e_ctrl"], image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    with pipe.open_session(slots=2, **SIZE, controlnet_conditioning_scale=0.8, compact=True) as ses:
        with pytest.raises(ValueError, match="pose_image"):
            ses.submit(**_submit_kw(reqs, 0, steps[0], guidance=gs, image_scale=(1.0, 1.0)))
        a = ses.submit(**_submit_kw(reqs, 0, steps[0], guidance=gs, image_scale=(1.0, 1.0), pose_image=pose[0].cuda()))
        ses.step(), ses.step()
        b = ses.submit(**_submit_kw(reqs, 1, steps[1], guidance=gs, image_scale=(1.0, 1.0), pose_image=pose[1].cuda()))
        ses.step()
        assert ses.width == 2 and ses.rows == [0, 1] and ses.repacks == 1
        for _ in range(5):
            ses.step()
        assert a.done and not b.done and ses.rows == [None, 1]
        ses.step()
        assert ses.width == 1 and ses.rows == [1] and ses.repacks == 2          # the survivor, slot 1, now in row 0
        ses.drain()
        assert (a.slot, b.slot) == (0, 1) and ses.steps_run == 10 and ses.steps_at_width == {1: 4, 2: 6}
    for r, t in enumerate((a, b)):
        st = _check(t.result().images, _CTRL_REF[r], _traj_bar(dtype), floor=1.0)
        print(f"controlnet compact session request {r} [{dtype}]: {st}")


@torch.no_grad()
def test_compact_session_life_cycle(small_pair):
    p, reqs = small_pair, _Requests()
    pipe = _pipe(p, _engine_scheduler("dpm"))
    call = dict(num_inference_steps=6, **reqs.solo_kwargs(0))
    before = pipe(**call).images
    unet = p["e_unet"]
    with pytest.raises(ValueError, match="widths"):
        pipe.open_session(slots=2, **SIZE, compact=True, widths=(1,))
    ses = pipe.open_session(slots=2, **SIZE, compact=True)
    assert ses.step() == [] and ses.steps_run == 0 and ses.width == 0 and ses.rows == [] and ses.steps_at_width == {}
    with pytest.raises(NotImplementedError, match="guidance_scale <= 1"):
        ses.submit(**_submit_kw(reqs, 0, 6, guidance=(1.0, 1.0, 1.0)))
    with pytest.raises(ValueError, match="one geometry per session"):
        ses.submit(**_submit_kw(reqs, 0, 6, latents=torch.zeros(1, 4, 16, 24).cuda()))
    # a failed admission: the request leaves, the one behind it runs alone at width 1
    bad = ses.submit(**_submit_kw(reqs, 0, 4, prompt_embeds=torch.zeros(2, 77, 64).cuda()))
    good = ses.submit(**_submit_kw(reqs, 1, 3))
    with pytest.raises(ValueError, match="one prompt"):
        ses.step()
    assert bad.error is not None and ses.steps_run == 0
    ses.step()
    assert ses.width == 1 and ses.rows == [good.slot] and ses.repacks == 0
    assert ses.drain() == [good] and ses.steps_at_width == {1: 3}
    # a request of two images takes two slots and two rows
    two = ses.submit(**_submit_kw(reqs, 1, 5, latents=torch.cat([reqs.latent(1, 0), reqs.latent(1, 1)]).cuda(), num_images_per_prompt=2))
    one = ses.submit(**_submit_kw(reqs, 0, 3))
    assert ses.step() == [] and two.slots == [0, 1] and ses.rows == [0, 1] and ses.width == 2 and one.slot is None
    assert ses.drain() == [two, one] and ses.steps_run == 3 + 5 + 3
    assert two.result().images.shape == (2, 4, 16, 16) and not torch.equal(two.result().images[0], two.result().images[1])
    # a step that raises: the encoders' time-embedding state does not leak out of it, and close() drops the unfinished ticket
    t = ses.submit(**_submit_kw(reqs, 2, 4))
    real = unet.forward_nhwc

    def boom(*a, **k):
        assert unet.__dict__.get("_temb_fixed") is not None
        raise RuntimeError("boom")
    unet.forward_nhwc = boom
    try:
        with pytest.raises(RuntimeError, match="boom"):
            ses.step()
    finally:
        unet.forward_nhwc = real
    assert unet.__dict__.get("_temb_fixed") is None and unet.__dict__.get("_temb_table") is None
    ses.step()                                                            # the session goes on
    assert not t.done and ses.width == 1
    ses.close()
    assert ses.closed and ses.z is None and ses.row_slot is None
    with pytest.raises(RuntimeError, match="closed"):
        ses.step()
    with pytest.raises(RuntimeError, match="dropped"):
        t.result()
    ses.close()                                                           # idempotent
    after = pipe(**call).images
    assert torch.equal(before, after)
