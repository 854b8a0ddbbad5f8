"""The host side of in-flight batching without a GPU: ``session.SessionPlan`` -- slots, the queue, one scheduler / history / position
per request, one coefficient row and timestep per slot and step -- the DDIM row against the oracle's step, and the refusals."""
import pytest
import torch

from imagdressing_amd import ops
from imagdressing_amd import scheduler as S
from imagdressing_amd.session import SessionPlan, check_pipeline, check_request, check_scheduler

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _mk(name):
    return {"dpm": lambda: S.DPMSolverMultistepScheduler(**KW), "euler": lambda: S.EulerDiscreteScheduler(**KW),
            "euler_a": lambda: S.EulerAncestralDiscreteScheduler(**KW), "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW),
            "unipc": lambda: S.UniPCMultistepScheduler(**KW),
            "ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW)}[name]()


def _solo(name, n):
    """the request's own run: SamplerHistory(...).coefs(plan(i)) for every UNet call, and its timesteps"""
    sch = _mk(name)
    sch.set_timesteps(n)
    ring = S.SamplerHistory(sch.history)
    return [ring.coefs(sch.plan(i)) for i in range(sch.steps())], [t.item() for t in sch.timesteps]


def _drive(plan, arrivals=None, limit=200):
    """step the plan until it is empty -> per run: [(step, slot, row16, timestep)]; per step: the rows of all slots.
    ``arrivals`` = {step: [(steps, tag)]} submitted before that step's admission."""
    seen, steps, runs = {}, [], {}
    k = 0
    while plan.running or plan.pending or any(s >= k for s in (arrivals or {})):
        for n, tag in (arrivals or {}).get(k, []):
            runs[tag] = plan.submit(n, payload=tag)
        plan.admit()
        if not plan.running:
            k += 1
            continue
        st = plan.next_rows()
        steps.append(st)
        for slot, run, i in st.running:
            seen.setdefault(run.payload, []).append((k, slot, st.rows[slot], st.timesteps[slot], i))
        k += 1
        assert k < limit
    return seen, steps, runs


@pytest.mark.parametrize("name", ["dpm", "euler", "pndm"])
def test_every_request_runs_its_own_coefficient_sequence(name):
    """12, 8 and 10 steps on 2 slots (the third queued): each request gets exactly the rows and timesteps of its own solo run, free
    slots are inactive rows, the queued request inherits the slot that frees first and starts with every history coefficient 0."""
    sch = _mk(name)
    sch.set_timesteps(50)                     # the pipeline's scheduler keeps whatever schedule it had: the plan never touches it
    before = [t.item() for t in sch.timesteps]
    plan = SessionPlan(2, sch)
    assert plan.K == sch.history
    wants = {"a": 12, "b": 8, "c": 10}
    seen, steps, runs = _drive(plan, {0: [(12, "a"), (8, "b"), (10, "c")]})
    assert [t.item() for t in sch.timesteps] == before and all(r.scheduler is not sch for r in runs.values())
    calls = {tag: len(_solo(name, n)[0]) for tag, n in wants.items()}          # PNDM: n + 1 UNet calls
    for tag, n in wants.items():
        rows, ts = _solo(name, n)
        got = seen[tag]
        assert len(got) == calls[tag] == runs[tag].steps
        assert [g[2][:13] for g in got] == rows, tag                             # exactly: the same float64 -> float values
        assert [g[3] for g in got] == ts, tag
        assert all(g[2][13] == 1.0 and g[2][14:] == [0.0, 0.0] for g in got)
        assert [g[4] for g in got] == list(range(calls[tag]))
        assert [g[0] for g in got] == list(range(got[0][0], got[0][0] + calls[tag]))      # consecutive steps, no gap
    # slots lowest first; the queued request enters the slot that "b" left, at the step after b's last
    assert {g[1] for g in seen["a"]} == {0} and {g[1] for g in seen["b"]} == {1} and {g[1] for g in seen["c"]} == {1}
    assert seen["a"][0][0] == seen["b"][0][0] == 0 and seen["c"][0][0] == calls["b"]
    first = seen["c"][0][2]
    assert first[4:8] == [0.0] * 4                                                # a reused slot's first row reads no history
    # free slots are inactive rows with no timestep: after "a" ends slot 0 idles while "c" still runs
    end_a, end_c = calls["a"], calls["b"] + calls["c"]
    assert len(steps) == end_c
    for k in range(end_a, end_c):
        assert steps[k].rows[0][13] == 0.0 and steps[k].timesteps[0] is None and steps[k].rows[1][13] == 1.0
    assert steps[0].rows[0][13] == steps[0].rows[1][13] == 1.0
    # finished is reported with the last step, and the slot is free from the next one on
    assert [r.payload for r in steps[calls["b"] - 1].finished] == ["b"] and [r.payload for r in steps[end_a - 1].finished] == ["a"]
    assert plan.running == 0 and plan.pending == 0 and plan.free_slots == [0, 1]


def test_ddim_plan_rows():
    """DDIM in a plan: no history slots, rows from ddim_row at the request's own timesteps, m = e"""
    sch = _mk("ddim")
    plan = SessionPlan(2, sch)
    assert plan.K == 0
    seen, steps, runs = _drive(plan, {0: [(12, "a"), (8, "b")], 3: [(10, "c")]})
    for tag, n in (("a", 12), ("b", 8), ("c", 10)):
        solo = _mk("ddim")
        solo.set_timesteps(n)
        ts = [int(t) for t in solo.timesteps]
        assert [g[3] for g in seen[tag]] == ts
        for g, t in zip(seen[tag], ts):
            row = S.ddim_row(solo, t)
            assert g[2][:13] == ops.sampler_coefs(0.0, 1.0, row.z_x, row.z_m, (), 0.0, 1.0, 0.0, 1.0, -1)
    assert seen["c"][0][0] == 8 and {g[1] for g in seen["c"]} == {1}          # submitted at step 3, waits for b's slot


def test_slots_lowest_first_and_queue_fifo():
    plan = SessionPlan(3, _mk("euler"))
    a, b, c = plan.submit(2, "a"), plan.submit(5, "b"), plan.submit(3, "c")
    assert [r.payload for r in plan.admit()] == ["a", "b", "c"] and (a.slot, b.slot, c.slot) == (0, 1, 2)
    d, e, f = plan.submit(2, "d"), plan.submit(2, "e"), plan.submit(2, "f")
    assert plan.admit() == [] and plan.pending == 3
    plan.next_rows()
    assert plan.admit() == []
    st = plan.next_rows()                                  # a finishes: slot 0 is free from the next step on
    assert [r.payload for r in st.finished] == ["a"]
    assert [r.payload for r in plan.admit()] == ["d"] and d.slot == 0 and plan.pending == 2
    st = plan.next_rows()                                  # c finishes (3 steps)
    assert [r.payload for r in st.finished] == ["c"]
    assert [r.payload for r in plan.admit()] == ["e"] and e.slot == 2
    st = plan.next_rows()                                  # d finishes
    assert [r.payload for r in st.finished] == ["d"]
    assert [r.payload for r in plan.admit()] == ["f"] and f.slot == 0          # the lowest free slot, not the most recent
    plan.cancel(f)
    assert plan.free_slots == [0]


def test_ddim_row_equals_the_oracle_step_in_float64():
    """z' = row applied in float64 == oracle.ddim.DDIMOracle.step over a whole 20-step schedule, 1e-12 relative.  The oracle keeps its
    alphas as fp32 tensors and would take their square roots in fp32; for a float64 comparison it is handed the same fp32 VALUES
    widened to float64 (what ``DDIMScheduler.alpha`` returns), so both sides evaluate the same formula on the same numbers."""
    from oracle.ddim import DDIMOracle
    from tests.sampler_oracle import apply_row
    assert not hasattr(S.DDIMScheduler, "plan")          # the pipelines' loop picks the fused-sampler path by that attribute
    sch = _mk("ddim")
    sch.set_timesteps(20)
    orc = DDIMOracle()
    orc.alphas_cumprod = orc.alphas_cumprod.double()
    orc.final_alpha_cumprod = orc.final_alpha_cumprod.double()
    ts = orc.set_timesteps(20)
    assert [int(t) for t in ts] == [int(t) for t in sch.timesteps]
    gen = torch.Generator().manual_seed(3)
    z_row = z_orc = torch.randn(2, 64, 4, generator=gen, dtype=torch.float64)
    for t in ts:
        e = torch.randn(2, 64, 4, generator=gen, dtype=torch.float64)
        row = S.ddim_row(sch, int(t))
        assert (row.m_x, row.m_e, row.keep, row.z_h, row.in_scale) == (0.0, 1.0, False, (), 1.0)
        one = apply_row(row, z_orc, e, [])               # the same input: the step alone
        z_orc = orc.step(e, t, z_orc)
        z_row = apply_row(row, z_row, e, [])             # and the trajectory
        assert z_orc.dtype == torch.float64
        scale = z_orc.abs().max().item()
        assert (one - z_orc).abs().max().item() <= 1e-12 * scale, int(t)
        assert (z_row - z_orc).abs().max().item() <= 1e-12 * scale, int(t)


# ---- refusals ----
def test_scheduler_refusals():
    with pytest.raises(NotImplementedError, match="UniPC"):
        SessionPlan(2, _mk("unipc"))
    with pytest.raises(NotImplementedError, match="Euler-ancestral"):
        SessionPlan(2, _mk("euler_a"))
    with pytest.raises(NotImplementedError, match="affine step row"):
        check_scheduler(object())
    for ok in ("dpm", "euler", "pndm", "ddim"):
        check_scheduler(_mk(ok))
    with pytest.raises(ValueError, match="slots"):
        SessionPlan(0, _mk("dpm"))


def test_request_refusals():
    ok = dict(size=(128, 128), num_inference_steps=10, guidance_scale=7.5, slots=2)
    check_request(**ok)
    check_request(width=128, height=128, num_images_per_prompt=2, **ok)
    for over, exc, word in ((dict(eta=0.5), NotImplementedError, "eta > 0"),
                            (dict(shard_over_ranks=True), NotImplementedError, "shard_over_ranks"),
                            (dict(width=192), ValueError, "width x height"), (dict(height=64), ValueError, "width x height"),
                            (dict(control_guidance_start=0.2), NotImplementedError, "control_guidance_start"),
                            (dict(control_guidance_end=0.8), NotImplementedError, "control_guidance_start / control_guidance_end"),
                            (dict(guidance_scale=1.0), NotImplementedError, "guidance_scale <= 1"),
                            (dict(guidance_scale=[5.0, 7.0]), ValueError, "guidance_scale is per request"),
                            (dict(num_inference_steps=0), ValueError, "num_inference_steps"),
                            (dict(num_images_per_prompt=3), ValueError, "num_images_per_prompt")):
        with pytest.raises(exc, match=word):
            check_request(**dict(ok, **over))


def test_pipeline_refusals_precede_any_device_work():
    """enable_deepcache on: open_session raises before it allocates (these pipelines have no models at all); the IP-Adapter and
    inpainting pipelines have no session yet"""
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline as base
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet as ctrl
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet_inpainting as inp
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_ipa_controlnet as ipa
    kw = dict(vae=None, reference_unet=None, unet=None, tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None)
    for pipe in (base.IMAGDressing_v1(scheduler=_mk("dpm"), **kw), ctrl.IMAGDressing_v1(scheduler=_mk("dpm"), controlnet=None, **kw)):
        pipe.enable_deepcache(3)
        with pytest.raises(NotImplementedError, match="enable_deepcache"):
            pipe.open_session(slots=2, width=128, height=128)
        pipe.disable_deepcache()
        check_pipeline(pipe)
    for name in ("unipc", "euler_a"):
        with pytest.raises(NotImplementedError, match="open_session: scheduler"):
            base.IMAGDressing_v1(scheduler=_mk(name), **kw).open_session(slots=2, width=128, height=128)
    for mod in (inp, ipa):
        with pytest.raises(NotImplementedError, match="open_session"):
            mod.IMAGDressing_v1.open_session(object.__new__(mod.IMAGDressing_v1), slots=2, width=128, height=128)
