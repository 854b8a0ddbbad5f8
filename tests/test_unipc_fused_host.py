"""UniPC on the fused step without a GPU: ``UniPCMultistepScheduler.plan_fused`` + ``UniPCHistory`` -- one 19-value coefficient block
per step, two stores -- emulated with numpy exactly as ``imd_unipc_step`` evaluates it (m, then s' from m, then z' from the s' just
computed, then the blend on z' alone) against oracle/unipc.py, the library-form restatement in float64; the slot bookkeeping; the
session plan; the switch."""
import numpy as np
import pytest
import torch

from imagdressing_amd import ops
from imagdressing_amd import scheduler as S
from imagdressing_amd.session import SessionPlan, check_scheduler
from oracle.unipc import UniPCOracle
from tests.test_session_host import KW, _drive

T = 1000


class SpacedOracle(UniPCOracle):
    """the oracle with the library's other two timestep spacings (its own ``set_timesteps`` knows "linspace" only) and a start at a
    later schedule position -- the state ``step`` keeps is untouched"""

    def __init__(self, spacing="linspace", **kw):
        super().__init__(**kw)
        self.spacing = spacing

    def set_timesteps(self, n, t_start=0):
        super().set_timesteps(n)
        if self.spacing != "linspace":
            if self.spacing == "leading":
                ts = (np.arange(0, n + 1) * (self.T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64)
            else:
                ts = (np.arange(self.T, 0, -self.T / n).round() - 1).astype(np.int64)
            ac = self.alphas_cumprod
            sig = ((1 - ac) / ac) ** 0.5
            self.sigmas = np.concatenate([sig[ts], sig[:1]])
            self.timesteps = torch.from_numpy(ts)
        self.step_index = int(t_start)          # diffusers' _init_step_index of a run that begins at timesteps[t_start]
        return self.timesteps


def emulate(c, z, e, hist, blend=None):
    """one ``imd_unipc_step`` on float64 arrays: c = the 19 values of ops.unipc_coefs, hist [4, ...] by physical slot (updated in
    place, reads before stores) -> (z', m, s')"""
    m = c[0] * z + c[1] * e
    s = c[2] * z + c[3] * m + sum(c[4 + k] * hist[k] for k in range(4))
    zn = c[8] * s + c[9] * m + sum(c[10 + k] * hist[k] for k in range(4))
    if blend is not None:
        mask, z_img, noise = blend
        zn = (1.0 - mask) * (c[14] * z_img + c[15] * noise) + mask * zn
    sm, ss = int(c[17]), int(c[18])
    if sm >= 0:
        hist[sm] = m
    if ss >= 0:
        hist[ss] = s
    return zn, m, s


def eps_model(W):
    return lambda x, pos: np.tanh(x @ W + 0.1 * pos) + 0.05 * x          # smooth, nonlinear in x, different at every step


CASES = [dict(order=o) for o in (1, 2, 3)] + [
    dict(order=2, solver_type="bh1"), dict(order=3, solver_type="bh1"),
    dict(order=2, lower_order_final=False), dict(order=3, lower_order_final=False),
    dict(order=2, disable_corrector=(0, 4)), dict(order=3, disable_corrector=(2,)),
    dict(order=2, spacing="leading"), dict(order=3, spacing="trailing"), dict(order=3, spacing="leading", solver_type="bh1"),
]


def _pair(case, N, t_start):
    case = dict(case)
    order, spacing = case.pop("order"), case.pop("spacing", "linspace")
    sch = S.UniPCMultistepScheduler(solver_order=order, timestep_spacing=spacing, fused_step=True, **case, **KW)
    sch.set_timesteps(N)
    orc = SpacedOracle(spacing=spacing, solver_order=order, **case)
    ts = orc.set_timesteps(N, t_start)
    assert [int(t) for t in sch.timesteps] == [int(t) for t in ts]
    return sch, orc, ts, order


@pytest.mark.parametrize("t_start", [0, 3])
@pytest.mark.parametrize("N", [10, 25])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_fused_rows_equal_the_library_form_oracle(case, N, t_start):
    """whole runs on random vectors with a synthetic epsilon function; the first step's last_sample is the input z (s_x = 1)"""
    rng = np.random.default_rng(7)
    f = eps_model(rng.standard_normal((6, 6)) * 0.4)
    sch, orc, ts, order = _pair(case, N, t_start)
    assert sch.history == order + 1 and sch.steps(t_start) == N - t_start and sch.input_scale(0) == 1.0
    x0 = rng.standard_normal((2, 6))
    xo, z = torch.from_numpy(x0.copy()), x0.copy()
    hist, ring = np.full((4, 2, 6), np.nan), S.UniPCHistory(sch.history)          # (NaN: a slot read before it was written would show)
    hist[:] = 0.0
    for i in range(N - t_start):
        row = sch.plan_fused(i, t_start)
        if i == 0:
            assert (row.s_x, row.s_m, row.s_l, set(row.s_h) <= {0.0}) == (1.0, 0.0, 0.0, True)
        c = ring.coefs(row)
        xo = orc.step(torch.from_numpy(f(xo.numpy(), i)), ts[t_start + i], xo)
        z, m, s = emulate(c, z, f(z, i), hist)
        scale = np.abs(xo.numpy()).max()
        assert np.abs(z - xo.numpy()).max() <= 1e-12 * scale, (i, np.abs(z - xo.numpy()).max(), scale)
        assert np.abs(s - orc.last_sample.numpy()).max() <= 1e-12 * np.abs(orc.last_sample.numpy()).max(), i
        assert np.abs(m - orc.model_outputs[-1].numpy()).max() <= 1e-12 * max(np.abs(orc.model_outputs[-1].numpy()).max(), scale), i
    # plan_fused is a pure function of the positions: the instance's running state was never touched
    assert sch.step_index == 0 and sch.model_outputs == [] and sch.last_sample is None


@pytest.mark.parametrize("t_start", [0, 3])
@pytest.mark.parametrize("order", [2, 3])
def test_fused_rows_with_a_blend_between_steps(order, t_start):
    """the inpainting loop: the caller blends the oracle's output toward the image latents re-noised to the NEXT timestep (the clean
    image after the last step) and hands the blended sample to the next step; the oracle's own last_sample stays unblended -- in the
    kernel's form the blend touches z' only, never s'"""
    rng = np.random.default_rng(11)
    f = eps_model(rng.standard_normal((6, 6)) * 0.4)
    N = 10
    sch, orc, ts, _ = _pair(dict(order=order), N, t_start)
    x0, z_img, noise = rng.standard_normal((3, 2, 6))
    mask = rng.choice([0.0, 1.0, 0.5], size=(2, 6))
    xo, z = torch.from_numpy(x0.copy()), x0.copy()
    hist, ring = np.zeros((4, 2, 6)), S.UniPCHistory(sch.history)
    for i in range(N - t_start):
        pos = t_start + i
        c = ring.coefs(sch.plan_fused(i, t_start, blend=True))
        xo = orc.step(torch.from_numpy(f(xo.numpy(), i)), ts[pos], xo)
        proper = z_img if pos == N - 1 else orc.add_noise(z_img, noise, ts[pos + 1])
        unblended = xo.numpy().copy()
        xo = torch.from_numpy((1.0 - mask) * proper + mask * xo.numpy())
        z, m, s = emulate(c, z, f(z, i), hist, blend=(mask, z_img, noise))
        scale = np.abs(xo.numpy()).max()
        assert np.abs(z - xo.numpy()).max() <= 1e-12 * scale, (i, np.abs(z - xo.numpy()).max())
        assert np.abs(s - orc.last_sample.numpy()).max() <= 1e-12 * np.abs(orc.last_sample.numpy()).max(), i
        assert not np.array_equal(unblended, xo.numpy())
    assert np.array_equal(z[mask == 0.0], z_img[mask == 0.0])          # the clean image after the last step, exactly
    # without blend= the block is the identity pair the kernel ignores (no mask)
    assert (sch.plan_fused(0).b_img, sch.plan_fused(0).b_noise) == (1.0, 0.0)


@pytest.mark.parametrize("t_start", [0, 3])
@pytest.mark.parametrize("N", [4, 10, 25])
@pytest.mark.parametrize("case", [dict(order=1), dict(order=2), dict(order=3), dict(order=3, lower_order_final=False),
                                  dict(order=3, disable_corrector=(1, 2, 5))], ids=str)
def test_slot_bookkeeping(case, N, t_start):
    """what every physical slot holds is tracked by name: the step reads x0 prediction pos-1-j from the slot of age j and last_sample
    from its own slot -- never a slot that was recycled --, store_m != store_s at every step, and K = order + 1 slots suffice"""
    case = dict(case)
    order = case.pop("order")
    sch = S.UniPCMultistepScheduler(solver_order=order, fused_step=True, **case, **KW)
    sch.set_timesteps(N)
    K = sch.history
    assert K == order + 1 <= ops.SAMPLER_MAX_HISTORY
    ring, content = S.UniPCHistory(K), {}
    for i in range(N - t_start):
        pos = t_start + i
        row = sch.plan_fused(i, t_start)
        assert len(row.s_h) == len(row.z_h) == order
        slots_before, last = list(ring.slots), ring.last
        c = ring.coefs(row)
        sh, zh, sm, ss = c[4:8], c[10:14], int(c[17]), int(c[18])
        assert sm != ss and 0 <= sm < K and 0 <= ss < K and ss == last
        assert all(v == 0.0 for v in sh[K:] + zh[K:])
        for k in range(4):          # every slot the launch reads holds exactly what the row means by it
            if sh[k] != 0.0 or zh[k] != 0.0:
                if k == last:
                    assert content[k] == ("s", pos - 1) and sh[k] == row.s_l and zh[k] == 0.0
                else:
                    j = slots_before.index(k)
                    assert content[k] == ("m", pos - 1 - j), (i, k, content)
                    assert sh[k] == row.s_h[j] and zh[k] == row.z_h[j]
        for j, v in enumerate(row.s_h):
            assert v == 0.0 or sh[slots_before[j]] == v
        for j, v in enumerate(row.z_h):
            assert v == 0.0 or zh[slots_before[j]] == v
        if i > 0 and (pos - 1) not in sch.disable_corrector:
            assert row.s_x == 0.0 and row.s_l != 0.0 and row.s_m != 0.0
        else:
            assert (row.s_x, row.s_l, row.s_m) == (1.0, 0.0, 0.0) and set(row.s_h) <= {0.0}
        content[sm], content[ss] = ("m", pos), ("s", pos)
        assert ring.slots[0] == sm and len(set(ring.slots + [ring.last])) == len(ring.slots) + 1 <= K
    with pytest.raises(ValueError, match="only 0 are stored"):
        S.UniPCHistory(3).coefs(S.UniPCRow(z_h=(0.5,)))
    with pytest.raises(ValueError, match="K = 1"):
        S.UniPCHistory(1)


def _solo(order, n):
    sch = S.UniPCMultistepScheduler(solver_order=order, fused_step=True, **KW)
    sch.set_timesteps(n)
    ring = S.UniPCHistory(sch.history)
    return [ring.coefs(sch.plan_fused(i)) for i in range(sch.steps())], [t.item() for t in sch.timesteps]


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("order", [2, 3])
def test_session_plan_rows_equal_the_solo_rows(order, compact):
    """requests admitted at different steps, with other step counts, on 2 slots (one queued): every request gets exactly the 24-float
    rows and the timesteps of its own solo run -- in the compacting plan too, by slot and by batch row"""
    sch = S.UniPCMultistepScheduler(solver_order=order, fused_step=True, **KW)
    sch.set_timesteps(50)
    before = [int(t) for t in sch.timesteps]
    plan = SessionPlan(2, sch, compact=compact)
    assert plan.K == order + 1 and plan.unipc and plan.row_floats == ops.UNIPC_ROW_FLOATS == 24 and len(plan.idle_row) == 24
    assert plan.idle_row[19] == 0.0
    wants = {"a": 12, "b": 8, "c": 10}
    seen, steps, runs = _drive(plan, {0: [(12, "a")], 2: [(8, "b"), (10, "c")]})
    assert [int(t) for t in sch.timesteps] == before and sch.step_index == 0 and all(r.scheduler is not sch for r in runs.values())
    for tag, n in wants.items():
        rows, ts = _solo(order, n)
        got = seen[tag]
        assert len(got) == n == runs[tag].steps
        assert [g[2][:19] for g in got] == rows, tag                             # exactly: the same float64 -> float values
        assert [g[3] for g in got] == ts, tag
        assert all(g[2][19] == 1.0 and g[2][20:] == [0.0] * 4 for g in got)
        assert [g[0] for g in got] == list(range(got[0][0], got[0][0] + n))      # consecutive steps, no gap
    assert seen["a"][0][0] == 0 and seen["b"][0][0] == 2 and seen["c"][0][0] == 2 + 8          # c waits for b's slot
    for st in steps:
        assert st.width == len(st.coef_rows) == len(st.row_slot)
        for r, s in enumerate(st.row_slot):
            assert st.coef_rows[r] == (st.rows[s] if s >= 0 else plan.idle_row)
            assert all(len(row) == 24 for row in st.coef_rows)
    if compact:
        assert {st.width for st in steps} == {1, 2}
    # the request's in_scale for session_input_rows comes from its own block
    assert runs["a"].in_scale == 1.0 and ops.unipc_coefs()[ops.UNIPC_IN_SCALE] == 1.0


def test_the_switch():
    """off (the default): the class is what it was -- no session, one guidance scale per call -- and ``plan_fused`` being there changes
    nothing; on: check_scheduler and the request checks pass"""
    from imagdressing_amd.dressing_sd.pipelines._base import request_count
    off = S.UniPCMultistepScheduler(**KW)
    assert off.fused_step is False and not hasattr(off, "plan") and hasattr(off, "plan_fused") and hasattr(off, "step_guided")
    assert not S.unipc_fused(off)
    with pytest.raises(NotImplementedError, match=r"open_session: scheduler UniPCMultistepScheduler \(UniPC\)"):
        check_scheduler(off)
    with pytest.raises(NotImplementedError, match="UniPC"):
        SessionPlan(2, off)
    args = dict(prompt=["a", "b", "c"], guidance_scale=[5.0, 7.5, 9.0])
    with pytest.raises(ValueError, match="UniPC takes one guidance scale per call"):
        request_count(args, scheduler=off)
    on = S.UniPCMultistepScheduler(fused_step=True, **KW)
    assert S.unipc_fused(on) and on.enable_fused_step() is on
    check_scheduler(on)
    assert request_count(args, scheduler=on) == 3
    assert SessionPlan(2, on).K == 3
    assert off.enable_fused_step() is off and S.unipc_fused(off)
    check_scheduler(off)
    off.disable_fused_step()
    assert not S.unipc_fused(off)
    with pytest.raises(NotImplementedError, match="UniPC"):
        check_scheduler(off)
    with pytest.raises(ValueError, match="outside the 10 steps"):
        on.set_timesteps(10) or on.plan_fused(8, 3)
    # a session keeps the setting it was opened with: a switch flipped under it is refused at the next submit
    plan = SessionPlan(2, on)
    plan.submit(4)
    on.disable_fused_step()
    with pytest.raises(RuntimeError, match="fused-step switch changed"):
        plan.submit(4)


def test_coefficient_block_layout():
    c = ops.unipc_coefs(1, 2, 3, 4, (5, 6), 7, 8, (9, 10, 11), 12, 13, 14, 2, 0)
    assert c == [1, 2, 3, 4, 5, 6, 0, 0, 7, 8, 9, 10, 11, 0, 12, 13, 14, 2, 0] and len(c) == ops.UNIPC_COEFS == 19
    assert ops.unipc_coefs() == [0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, -1, -1]          # s' = z, z' = s', nothing stored
    row = ops.unipc_coef_row(c)
    assert row[:19] == c and row[19:] == [1.0, 0.0, 0.0, 0.0, 0.0] and len(row) == ops.UNIPC_ROW_FLOATS
    assert ops.unipc_coef_row(c, active=False)[19] == 0.0
    with pytest.raises(ops.L.ImdError, match="history coefficients"):
        ops.unipc_coefs(s_h=(0,) * 5)
    with pytest.raises(ops.L.ImdError, match="19 values"):
        ops.unipc_coef_row(c[:13])


def test_exact_family_preconditions():
    """what tests/test_unipc_step_gpu.py::test_exact_family relies on: operands in {-2, 0, 2}, masks in {0, 1} and {0.5}, integer
    guidance, coefficients in {0, +-1/4, +-1/2, +-1, 2} with integer store slots in -1..K-1 that differ -- and then EVERY intermediate
    of the float64 evaluation (each product, each partial sum, the blend, the scaled UNet input) is exactly a float32, so the result
    does not depend on which multiply-adds are fused"""
    from tests.unipc_cases import EXACT_COEFS, EXACT_K, EXACT_SHAPES, EXACT_VALUES, exact_blocks, exact_operands, is_exact_fp32, step_ref
    names = set()
    for B, HW in EXACT_SHAPES:
        for K in EXACT_K:
            op = exact_operands(B, HW, K)
            for key in ("z", "eps", "H", "z_img", "bn"):
                assert set(op[key].unique().tolist()) <= set(EXACT_VALUES), key
            assert set(op["mask01"].unique().tolist()) <= {0.0, 1.0} and set(op["mask05"].unique().tolist()) == {0.5}
            assert all(float(v) == int(v) for v in op["g_rows"]) and len(op["g_rows"]) == B
            assert op["H"].shape[0] == K
            for name, c in exact_blocks(K):
                names.add(name)
                assert len(c) == ops.UNIPC_COEFS and set(c[:17]) <= set(EXACT_COEFS), (name, c)
                sm, ss = c[17], c[18]
                assert sm == int(sm) and ss == int(ss) and -1 <= sm < K and -1 <= ss < K and (sm != ss or sm == -1)
                if name.startswith("only"):          # an indicator: one coefficient of its group is non-zero
                    groups = (c[0:2], c[2:8], c[8:14])
                    assert any(sum(v != 0.0 for v in grp) == 1 for grp in groups), (name, c)
                for kind in (None, "mask01", "mask05"):
                    blend = None if kind is None else (op[kind], op["z_img"], op["bn"])
                    ref = step_ref(op["z"], op["eps"], op["g_rows"], c, op["H"], blend)
                    assert all(is_exact_fp32(t) for t in ref["parts"]), (B, HW, K, name, kind)
                    assert float(max(t.abs().max() for t in ref["parts"])) < 2.0 ** 12
    assert {"only s_h[3]", "only z_h[3]", "only s_x", "only s_m", "only z_s", "only z_m", "only m_x", "only m_e", "stores 1,0"} <= names
