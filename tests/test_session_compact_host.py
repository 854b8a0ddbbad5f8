"""The host side of a compacting session without a GPU: ``SessionPlan(..., compact=True, widths=...)`` -- slots stay the home of a
request, ROWS are positions of the batch the forward runs; the width ladder, when a step repacks and which row every slot gets."""
import random

import pytest

from imagdressing_amd import scheduler as S
from imagdressing_amd.session import SessionPlan, check_widths

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _mk(name="dpm"):
    return {"dpm": lambda: S.DPMSolverMultistepScheduler(**KW), "euler": lambda: S.EulerDiscreteScheduler(**KW),
            "ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW)}[name]()


def _drive(plan, arrivals, limit=300, each=None):
    """step the plan until it is empty -> the PlanSteps.  ``arrivals`` = {step: [(steps, tag)]}, submitted before that step's admission;
    ``each(plan, step, before)`` is called after every step with the width the plan had before it."""
    steps, runs, k = [], {}, 0
    while plan.running or plan.pending or any(s >= k for s in arrivals):
        for n, tag in arrivals.get(k, []):
            runs[tag] = plan.submit(n, payload=tag)
        plan.admit()
        if plan.running:
            before = plan.width
            st = plan.next_rows()
            steps.append(st)
            if each is not None:
                each(plan, st, before)
        k += 1
        assert k < limit
    return steps, runs


def _widths(steps):
    out = {}
    for st in steps:
        out[st.width] = out.get(st.width, 0) + 1
    return out


def test_staggered_trace_on_two_slots():
    """12 / 8 / 10 steps on 2 slots, the second and third submitted after step 3 (the third queued): 4 steps alone, 8 at width 2 --
    both end with step 11 --, then the third alone in slot 0"""
    plan = SessionPlan(2, _mk(), compact=True)
    steps, runs = _drive(plan, {0: [(12, "a")], 4: [(8, "b"), (10, "c")]})
    assert len(steps) == 22 and _widths(steps) == {1: 14, 2: 8} and plan.repacks == 2
    assert [k for k, st in enumerate(steps) if st.repack] == [4, 12]
    assert [st.width for st in steps] == [1] * 4 + [2] * 8 + [1] * 10
    assert steps[0].row_slot == [0] and steps[4].row_slot == [0, 1] and steps[12].row_slot == [0]
    assert (runs["a"].slot, runs["b"].slot, runs["c"].slot) == (0, 1, 0)
    for st in steps:                                       # per row: the slot's own coefficient row and timestep
        assert len(st.coef_rows) == len(st.row_timesteps) == len(st.row_slot) == st.width
        for r, s in enumerate(st.row_slot):
            assert st.coef_rows[r] == st.rows[s] and st.row_timesteps[r] == st.timesteps[s] and st.coef_rows[r][13] == 1.0


def test_shrink_moves_the_survivor_to_row_0():
    """4 / 9 / 6 steps on 3 slots, submitted together: widths 3,3,3,3,2,2,1,1,1; rows [1, 2] after the first repack, then [1]"""
    plan = SessionPlan(3, _mk("euler"), compact=True)
    steps, runs = _drive(plan, {0: [(4, "a"), (9, "b"), (6, "c")]})
    assert [st.width for st in steps] == [3, 3, 3, 3, 2, 2, 1, 1, 1]
    assert [st.repack for st in steps] == [False] * 4 + [True, False, True, False, False] and plan.repacks == 2
    assert steps[0].row_slot == [0, 1, 2] and steps[4].row_slot == [1, 2] and steps[5].row_slot == [1, 2] and steps[6].row_slot == [1]
    assert [runs[t].row for t in "abc"] == [0, 0, 1] and [runs[t].slot for t in "abc"] == [0, 1, 2]          # (the rows they ran in last)


def test_ladder_keeps_an_idle_row_and_refills_it():
    """widths (1, 2, 4) on 4 slots with 3 running: width 4, one idle row.  4 -> 3 running does not repack, the row idles with an
    inactive coefficient row, and the next admission takes exactly that row."""
    plan = SessionPlan(4, _mk(), compact=True, widths=(1, 2, 4))
    for n, tag in ((9, "a"), (3, "b"), (9, "c")):
        plan.submit(n, tag)
    plan.admit()
    st = plan.next_rows()
    assert st.width == 4 and st.row_slot == [0, 1, 2, -1] and not st.repack and st.coef_rows[3][13] == 0.0 and st.row_timesteps[3] is None
    d = plan.submit(9, "d")
    plan.admit()
    st = plan.next_rows()
    assert st.row_slot == [0, 1, 2, 3] and d.row == 3 and not st.repack          # 4 running
    st = plan.next_rows()                                  # "b" takes its last step
    assert [r.payload for r in st.finished] == ["b"] and st.row_slot == [0, 1, 2, 3]
    st = plan.next_rows()                                  # 3 running: no repack, row 1 idles
    assert st.width == 4 and not st.repack and st.row_slot == [0, -1, 2, 3] and plan.repacks == 0
    assert st.coef_rows[1][13] == 0.0 and st.row_timesteps[1] is None and all(st.coef_rows[r][13] == 1.0 for r in (0, 2, 3))
    e = plan.submit(2, "e")
    lay_before = plan.row_runs()
    assert [None if r is None else r.slot for r in lay_before] == [0, None, 2, 3]
    plan.admit()
    lay = plan.layout()
    assert lay.placed == [e] and not lay.repack and (e.slot, e.row) == (1, 1)
    st = plan.next_rows()
    assert st.row_slot == [0, 1, 2, 3] and not st.repack and plan.repacks == 0


def test_full_width_ladder_never_repacks():
    plan = SessionPlan(3, _mk(), compact=True, widths=(3,))
    steps, runs = _drive(plan, {0: [(5, "a")], 2: [(6, "b"), (2, "c"), (4, "d")]})
    assert plan.repacks == 0 and {st.width for st in steps} == {3} and not any(st.repack for st in steps)
    for st in steps:                                       # rows and slots fall free together: row == slot throughout
        assert all(s in (-1, r) for r, s in enumerate(st.row_slot))
    assert runs["d"].slot == runs["d"].row


@pytest.mark.parametrize("widths", [None, (1, 2, 4), (2, 4), (4,)])
def test_invariants_on_a_random_trace(widths):
    rng = random.Random(11)
    arrivals = {}
    for tag in range(40):
        arrivals.setdefault(rng.randrange(0, 90), []).append((rng.randrange(1, 12), tag))
    ladder = check_widths(4, widths)
    seen = {"first": True, "repacks": 0}

    def each(plan, st, before):
        live = [s for s, _, _ in st.running]
        named = [s for s in st.row_slot if s >= 0]
        assert sorted(named) == sorted(live) and len(set(named)) == len(named)          # every running slot in exactly one row
        for r, s in enumerate(st.row_slot):                                              # no idle row is active
            assert (st.coef_rows[r][13] == 1.0) == (s >= 0) and (st.row_timesteps[r] is None) == (s < 0)
        assert st.width == min(w for w in ladder if w >= len(live)) and len(st.row_slot) == st.width
        if seen["first"]:                                  # the first layout moves nothing
            assert not st.repack
            seen["first"] = False
        else:
            assert st.repack == (st.width != before)
        if st.repack:
            assert named == sorted(named) and st.row_slot[:len(named)] == named          # ascending slot order, idle rows last
            seen["repacks"] += 1
        assert plan.repacks == seen["repacks"]

    steps, runs = _drive(SessionPlan(4, _mk(), compact=True, widths=widths), arrivals, limit=600, each=each)
    assert len(runs) == 40 and all(r.done for r in runs.values())
    assert sum(len(st.finished) for st in steps) == 40
    if widths != (4,):
        assert seen["repacks"] > 0


def test_not_compact_is_todays_plan_step():
    """compact=False: the slot-indexed PlanStep of a plan built without the keyword, field for field, and the identity for the rest"""
    arrivals = {0: [(12, "a")], 4: [(8, "b"), (10, "c")]}
    old, _ = _drive(SessionPlan(2, _mk()), arrivals)
    new, _ = _drive(SessionPlan(2, _mk(), compact=False), arrivals)
    packed, _ = _drive(SessionPlan(2, _mk(), compact=True), arrivals)
    assert len(old) == len(new) == len(packed) == 22
    for a, b, c in zip(old, new, packed):
        assert a.rows == b.rows == c.rows and a.timesteps == b.timesteps == c.timesteps
        assert [(s, r.payload, i) for s, r, i in a.running] == [(s, r.payload, i) for s, r, i in b.running] == [(s, r.payload, i) for s, r, i in c.running]
        assert [r.payload for r in a.finished] == [r.payload for r in b.finished] == [r.payload for r in c.finished]
        assert b.width == 2 and b.row_slot == [0, 1] and not b.repack and b.coef_rows == b.rows and b.row_timesteps == b.timesteps
    plan = SessionPlan(2, _mk())
    assert not plan.compact and plan.widths == (2,) and plan.width == 2 and plan.repacks == 0


def test_in_scale_follows_the_last_coefficient_row():
    """what a repack re-lays a request's input with: first_input_scale() before its first step, coefficient [11] of its last after"""
    plan = SessionPlan(1, _mk("euler"), compact=True)
    run = plan.submit(5)
    assert run.in_scale == run.first_input_scale() != 1.0
    plan.admit()
    for _ in range(3):
        st = plan.next_rows()
        assert run.in_scale == st.coef_rows[0][11]


def test_bad_widths():
    for bad in ((), (1, 2), (2, 1, 4), (1, 1, 4), (0, 4), (1, 5), (1, 2.0, 4), "124", 4, (True, 4)):
        with pytest.raises(ValueError, match="widths"):
            SessionPlan(4, _mk(), compact=True, widths=bad)
    with pytest.raises(ValueError, match="widths"):
        SessionPlan(4, _mk(), compact=False, widths=(1, 4))
    assert SessionPlan(4, _mk(), compact=True).widths == (1, 2, 3, 4)
    assert SessionPlan(4, _mk(), compact=True, widths=[2, 4]).widths == (2, 4)


def test_open_session_takes_the_keywords():
    """the refusal reaches the caller through both pipelines before anything is allocated (these pipelines have no models)"""
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline as base
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet as ctrl
    kw = dict(vae=None, reference_unet=None, unet=None, tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None)
    for pipe in (base.IMAGDressing_v1(scheduler=_mk(), **kw), ctrl.IMAGDressing_v1(scheduler=_mk(), controlnet=None, **kw)):
        with pytest.raises(ValueError, match="widths"):
            pipe.open_session(slots=4, width=128, height=128, compact=True, widths=(1, 3))
