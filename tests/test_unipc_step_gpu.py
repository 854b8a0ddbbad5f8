"""The fused UniPC step on the GPU (``imd_unipc_step`` / ``_rows`` / ``_rows_at``, csrc/unipc_step.hip), both element types:

* the EXACT family -- operands and coefficients chosen so that every intermediate is a small dyadic rational (tests/unipc_cases.py;
  the preconditions are asserted on the CPU in tests/test_unipc_fused_host.py): ``torch.equal`` against the float64 evaluation,
  whatever the compiler contracts;
* the PARITY family -- Gaussian operands and the real coefficient rows of a 10-step order-3 run, within 32 * 2^-24 * A, A the same
  expression on absolute values (derived: at most 24 rounded operations deep, not measured);
* the identities between the three forms, the skips of inactive rows and idle slots;
* the parent's route: one step, and whole 10-step runs, against the three ``imd_lincomb`` launches of the switch-off class."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.unipc_cases import (EXACT_K, EXACT_SHAPES, KW, exact_blocks, exact_operands, half_ulp, parity_bound,  # noqa: E402
                               step_ref)

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
SENTINEL_X = 7.0


def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def launch(dtype, z0, eps, H0, c, guidance, blend=None, form="scalar", device_coefs=False, x_next=True):
    """one launch on fresh device copies -> (z, H, x_next); ``form``: scalar | rows | rows_at (identity map)"""
    from imagdressing_amd import ops
    B, HW = z0.shape[0], z0.shape[1]
    z, H = z0.clone().cuda(), (H0.clone().cuda() if H0.shape[0] else None)
    xn = torch.full((2 * B, HW, 8), SENTINEL_X, dtype=dtype).cuda() if x_next else None
    kw = dict(mask=blend[0].cuda(), z_img=blend[1].cuda(), blend_noise=blend[2].cuda()) if blend is not None else {}
    gd = guidance.cuda() if isinstance(guidance, torch.Tensor) else guidance
    if form == "scalar":
        ops.unipc_step(z, eps.cuda(), xn, guidance=gd, coefs=torch.tensor(c, dtype=torch.float32).cuda() if device_coefs else c, hist=H, **kw)
    else:
        rows = torch.tensor([ops.unipc_coef_row(c)] * B, dtype=torch.float32).cuda()
        if form == "rows":
            ops.unipc_step_rows(z, eps.cuda(), xn, guidance=gd, coef_rows=rows, hist=H, **kw)
        else:
            ops.unipc_step_rows_at(z, eps.cuda(), xn, guidance=gd, coef_rows=rows, row_slot=torch.arange(B, dtype=torch.int32).cuda(), hist=H, **kw)
    torch.cuda.synchronize()
    return z, H, xn


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---- the exact family ----
@DTYPES
@pytest.mark.parametrize("K", EXACT_K)
@pytest.mark.parametrize("B,HW", EXACT_SHAPES)
def test_exact_family(B, HW, K, dtype):
    """z, both stored history slots, the untouched slots: ``torch.equal`` with the float64 evaluation; x_next: its 16-bit rounding,
    padded channels zero, both CFG halves the same.  Guidance per row (integers) in every launch; general blocks, and the indicator
    blocks that name a swapped coefficient or store."""
    op = exact_operands(B, HW, K)
    for name, c in exact_blocks(K):
        for kind in (None, "mask01", "mask05"):
            what = (B, HW, K, name, kind)
            blend = None if kind is None else (op[kind], op["z_img"], op["bn"])
            ref = step_ref(op["z"], op["eps"], op["g_rows"], c, op["H"], blend)
            z, H, xn = launch(dtype, op["z"], op["eps"], op["H"], c, op["g_rows"], blend)
            assert torch.equal(z.cpu().double(), ref["z"]), what
            sm, ss = int(c[17]), int(c[18])
            for k in range(K):
                want = ref["m"] if k == sm else ref["s"] if k == ss else op["H"][k].double()
                assert torch.equal(H[k].cpu().double(), want), (what, "slot", k)
            assert torch.equal(xn[:B, :, :4], ref["x"].float().cuda().to(dtype)), what
            assert torch.equal(xn[:B], xn[B:]) and not xn[..., 4:].any(), what
    # the same through the other two forms (one block is enough: the identities are tested below on Gaussian data)
    name, c = exact_blocks(K)[0]
    blend = (op["mask05"], op["z_img"], op["bn"])
    first = launch(dtype, op["z"], op["eps"], op["H"], c, op["g_rows"], blend)
    for form in ("rows", "rows_at"):
        assert same(first, launch(dtype, op["z"], op["eps"], op["H"], c, op["g_rows"], blend, form=form)), (B, HW, K, form)


# ---- the parity family ----
def _real_rows(order=3, steps=10, blend=False, start=0):
    from imagdressing_amd import scheduler as S
    sch = S.UniPCMultistepScheduler(solver_order=order, fused_step=True, **KW)
    sch.set_timesteps(steps)
    ring = S.UniPCHistory(sch.history)
    return [ring.coefs(sch.plan_fused(i, start, blend=blend)) for i in range(steps - start)]


@DTYPES
@pytest.mark.parametrize("B,HW", [(1, 1), (3, 77), (2, 300)], ids=["lone", "partial-block", "row-boundary"])
def test_parity_family(B, HW, dtype):
    """Gaussian operands, the ten coefficient rows of an order-3 run (ramp-up, full order, lower_order_final), with and without the
    blend.  fp32 outputs within 32 * 2^-24 * A of the float64 evaluation; x_next within half a unit in the last place of the element
    type at the reference plus that bound."""
    K = 4
    z0, eps, H0 = g(1, B, HW, 4), g(2, 2 * B, HW, 4), g(3, K, B, HW, 4)
    z_img, bn = g(5, B, HW, 4), g(6, B, HW, 4)
    mask = (torch.rand(B, HW, generator=torch.Generator().manual_seed(7)) > 0.4).float()
    mask[0, 0] = 0.25
    g_rows = torch.tensor([5.0, 7.5, 9.0][:B])
    worst = 0.0
    for use_blend in (False, True):
        blend = (mask, z_img, bn) if use_blend else None
        for i, c in enumerate(_real_rows(blend=use_blend)):
            what = (B, HW, use_blend, i)
            c32 = torch.tensor(c, dtype=torch.float32).double().tolist()          # the coefficients the kernel sees
            ref = step_ref(z0, eps, g_rows, c32, H0, blend)
            bound = parity_bound(z0, eps, g_rows, c32, H0, blend)
            z, H, xn = launch(dtype, z0, eps, H0, c, g_rows, blend)
            sm, ss = int(c[17]), int(c[18])
            assert sm != ss and 0 <= sm < K and 0 <= ss < K
            for got, key in ((z, "z"), (H[sm], "m"), (H[ss], "s")):
                err = (got.cpu().double() - ref[key]).abs()
                worst = max(worst, float((err / bound[key].clamp_min(1e-300)).max()))
                assert bool((err <= bound[key]).all()), (what, key, float(err.max()), float(bound[key].max()))
            for k in range(K):
                if k not in (sm, ss):
                    assert torch.equal(H[k].cpu(), H0[k]), (what, "slot", k)
            errx = (xn[:B, :, :4].cpu().double() - ref["x"]).abs()
            assert bool((errx <= half_ulp(ref["x"], dtype) + bound["x"]).all()), (what, "x_next", float(errx.max()))
            assert torch.equal(xn[:B], xn[B:]) and not xn[..., 4:].any(), what
    print(f"unipc_step parity[{dtype}, B={B}, HW={HW}]: worst error / bound = {worst:.3f}")


# ---- identities ----
@DTYPES
@pytest.mark.parametrize("B,HW", [(3, 77), (2, 300)], ids=["partial-block", "row-boundary"])
def test_identities_between_the_forms(B, HW, dtype):
    """device coefficients == host scalars; rows with every row equal and active == scalar; rows_at with the identity map and
    slots == B == rows; a uniform guidance array == scalar guidance; row b of a mixed-guidance launch == the scalar launch with g[b];
    without x_next the latent is the same"""
    K = 4
    z0, eps, H0 = g(1, B, HW, 4), g(2, 2 * B, HW, 4), g(3, K, B, HW, 4)
    blend = ((torch.rand(B, HW, generator=torch.Generator().manual_seed(7)) > 0.4).float(), g(5, B, HW, 4), g(6, B, HW, 4))
    g_rows = torch.tensor([5.0, 7.5, 9.0][:B])
    rows = _real_rows(blend=True)
    for c in (rows[0], rows[4], rows[9]):
        for bl in (None, blend):
            for guidance in (7.5, g_rows):
                ref = launch(dtype, z0, eps, H0, c, guidance, bl)
                assert same(ref, launch(dtype, z0, eps, H0, c, guidance, bl, device_coefs=True))
                assert same(ref, launch(dtype, z0, eps, H0, c, guidance, bl, form="rows"))
                assert same(ref, launch(dtype, z0, eps, H0, c, guidance, bl, form="rows_at"))
            scalar = launch(dtype, z0, eps, H0, c, 7.5, bl)
            assert same(scalar, launch(dtype, z0, eps, H0, c, torch.full((B,), 7.5), bl))
            mixed = launch(dtype, z0, eps, H0, c, g_rows, bl)
            for b in range(B):
                one = launch(dtype, z0, eps, H0, c, float(g_rows[b]), bl)
                assert torch.equal(one[0][b], mixed[0][b]) and torch.equal(one[1][:, b], mixed[1][:, b])
                assert torch.equal(one[2][b], mixed[2][b]) and torch.equal(one[2][B + b], mixed[2][B + b])
            bare = launch(dtype, z0, eps, H0, c, 7.5, bl, x_next=False)
            assert torch.equal(bare[0], scalar[0]) and torch.equal(bare[1], scalar[1])


@DTYPES
def test_inactive_rows_and_the_slot_map(dtype):
    """rows: an inactive row keeps sentinel bytes in z, every history plane and both halves of x_next, the active rows equal the
    scalar launch on them.  rows_at with a permuted map over 5 slots: slot-addressed tensors land where the map says, slots that no
    row names -- and the slot of a row whose block is inactive -- keep their bytes, an idle row (-1, or a slot past the end) writes
    nothing."""
    from imagdressing_amd import ops
    K, HW, S, B = 4, 77, 5, 4
    rows = _real_rows(blend=True)
    zs, Hs = g(1, S, HW, 4), g(3, K, S, HW, 4)                      # by slot
    mask = (torch.rand(S, HW, generator=torch.Generator().manual_seed(7)) > 0.4).float()
    z_img, bn = g(5, S, HW, 4), g(6, S, HW, 4)
    eps = g(2, 2 * B, HW, 4)                                        # by row
    g_rows = torch.tensor([5.0, 7.5, 9.0, 6.0])
    # -- rows: row 1 inactive
    cs = [rows[2], rows[5], rows[7], rows[9]]
    table = torch.tensor([ops.unipc_coef_row(c, active=(r != 1)) for r, c in enumerate(cs)], dtype=torch.float32).cuda()
    z, H = zs[:B].clone().cuda(), Hs[:, :B].clone().contiguous().cuda()
    xn = torch.full((2 * B, HW, 8), SENTINEL_X, dtype=dtype).cuda()
    kw = dict(mask=mask[:B].cuda(), z_img=z_img[:B].cuda(), blend_noise=bn[:B].cuda())
    ops.unipc_step_rows(z, eps.cuda(), xn, guidance=g_rows.cuda(), coef_rows=table, hist=H, **kw)
    torch.cuda.synchronize()
    assert torch.equal(z[1].cpu(), zs[1]) and torch.equal(H[:, 1].cpu(), Hs[:, 1])
    assert bool((xn[1] == SENTINEL_X).all()) and bool((xn[B + 1] == SENTINEL_X).all())
    solo = {}
    for r in (0, 2, 3):
        one = launch(dtype, zs[r:r + 1], torch.stack([eps[r], eps[B + r]]), Hs[:, r:r + 1].contiguous(), cs[r], float(g_rows[r]),
                     (mask[r:r + 1], z_img[r:r + 1], bn[r:r + 1]))
        solo[r] = one
        assert torch.equal(one[0][0], z[r]) and torch.equal(one[1][:, 0], H[:, r]), r
        assert torch.equal(one[2][0], xn[r]) and torch.equal(one[2][1], xn[B + r]), r
    # -- rows_at: row 0 -> slot 3, row 1 inactive (names slot 1), row 2 -> slot 0, row 3 idle; slots 1, 2, 4 keep their bytes
    for idle in (-1, S, 1 << 20):
        row_slot = torch.tensor([3, 1, 0, idle], dtype=torch.int32).cuda()
        z, H = zs.clone().cuda(), Hs.clone().cuda()
        xn = torch.full((2 * B, HW, 8), SENTINEL_X, dtype=dtype).cuda()
        ops.unipc_step_rows_at(z, eps.cuda(), xn, guidance=g_rows.cuda(), coef_rows=table, row_slot=row_slot, hist=H,
                               mask=mask.cuda(), z_img=z_img.cuda(), blend_noise=bn.cuda())
        torch.cuda.synchronize()
        for s in (1, 2, 4):
            assert torch.equal(z[s].cpu(), zs[s]) and torch.equal(H[:, s].cpu(), Hs[:, s]), (idle, s)
        for r in (1, 3):
            assert bool((xn[r] == SENTINEL_X).all()) and bool((xn[B + r] == SENTINEL_X).all()), (idle, r)
        for r, s in ((0, 3), (2, 0)):
            one = launch(dtype, zs[s:s + 1], torch.stack([eps[r], eps[B + r]]), Hs[:, s:s + 1].contiguous(), cs[r], float(g_rows[r]),
                         (mask[s:s + 1], z_img[s:s + 1], bn[s:s + 1]))
            assert torch.equal(one[0][0], z[s]) and torch.equal(one[1][:, 0], H[:, s]), (idle, r, s)
            assert torch.equal(one[2][0], xn[r]) and torch.equal(one[2][1], xn[B + r]), (idle, r, s)
    # device store slots outside 0..K-1 store nothing (the launcher never sees them)
    c = list(rows[5])
    c[17], c[18] = 4.0, -3.0
    out = launch(dtype, zs[:2], eps[:4], Hs[:, :2].contiguous(), c, 7.5, device_coefs=True)
    assert torch.equal(out[1].cpu(), Hs[:, :2]) and torch.isfinite(out[0]).all()


def test_launcher_refusals_leave_the_latent_alone():
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    B, HW = 2, 40
    z0, eps = g(1, B, HW, 4).cuda(), g(2, 2 * B, HW, 4).cuda()
    hist = torch.zeros(3, B, HW, 4).cuda()
    for kw, c, word in ((dict(hist=hist), ops.unipc_coefs(store_m=1, store_s=1), "the same slot 1"),
                        (dict(hist=hist), ops.unipc_coefs(store_m=3), "store_m slot 3"),
                        (dict(), ops.unipc_coefs(store_s=0), "store_s slot 0"),
                        (dict(hist=torch.zeros(5, B, HW, 4).cuda()), ops.unipc_coefs(), "K (5)"),
                        (dict(mask=torch.ones(B, HW).cuda()), ops.unipc_coefs(), "inpaint mask")):
        z = z0.clone()
        with pytest.raises(ImdError, match=word.replace("(", r"\(").replace(")", r"\)")):
            ops.unipc_step(z, eps, None, guidance=7.5, coefs=c, **kw)
        torch.cuda.synchronize()
        assert torch.equal(z, z0)


# ---- against the parent's route: the three imd_lincomb launches of the switch-off class ----
def _three_launch_state(order, steps, upto, B, HW, gs):
    """run the switch-off class for ``upto`` steps on fixed Gaussian epsilons -> (scheduler, z before step ``upto``, eps of it)"""
    from imagdressing_amd import scheduler as S
    sch = S.UniPCMultistepScheduler(solver_order=order, **KW)
    sch.set_timesteps(steps)
    z = g(1, B, HW, 4).cuda()
    for i in range(upto):
        z = sch.step_guided(g(100 + i, 2 * B, HW, 4, scale=0.8).cuda(), z, gs)
    return sch, z, g(100 + upto, 2 * B, HW, 4, scale=0.8).cuda()


@DTYPES
@pytest.mark.parametrize("at", [0, 1, 4, 9])
def test_one_step_against_the_three_launches(at, dtype):
    """step ``at`` of a 10-step order-3 run on the SAME operands (the three-launch route's own state laid into the history planes):
    both routes within the parity bound of the float64 evaluation -- the new latent, the stored x0 prediction and last_sample"""
    from imagdressing_amd import ops, scheduler as S
    B, HW, gs, order, steps = 2, 300, 7.5, 3, 10
    sch, z0, eps = _three_launch_state(order, steps, at, B, HW, gs)
    fused = S.UniPCMultistepScheduler(solver_order=order, fused_step=True, **KW)
    fused.set_timesteps(steps)
    ring = S.UniPCHistory(fused.history)
    for i in range(at):
        ring.coefs(fused.plan_fused(i))
    H0 = torch.zeros(fused.history, B, HW, 4).cuda()
    for slot, m in zip(ring.slots, reversed(sch.model_outputs)):          # newest first
        H0[slot].copy_(m)
    if sch.last_sample is not None:
        H0[ring.last].copy_(sch.last_sample)
    c = ring.coefs(fused.plan_fused(at))
    z, H, xn = z0.clone(), H0.clone(), torch.zeros(2 * B, HW, 8, dtype=dtype).cuda()
    ops.unipc_step(z, eps, xn, guidance=gs, coefs=c, hist=H)
    three = sch.step_guided(eps, z0, gs)                                    # x0 prediction, corrector, predictor: one launch each
    torch.cuda.synchronize()
    c32 = torch.tensor(c, dtype=torch.float32).double().tolist()
    g_rows = torch.full((B,), gs)
    ref = step_ref(z0.cpu(), eps.cpu(), g_rows, c32, H0.cpu())
    bound = parity_bound(z0.cpu(), eps.cpu(), g_rows, c32, H0.cpu())
    sm, ss = int(c[17]), int(c[18])
    for key, mine, theirs in (("z", z, three), ("m", H[sm], sch.model_outputs[-1]), ("s", H[ss], sch.last_sample)):
        e1, e3 = (mine.cpu().double() - ref[key]).abs(), (theirs.cpu().double() - ref[key]).abs()
        print(f"one step at {at} [{dtype}] {key}: fused {float((e1 / bound[key]).max()):.3f}, three launches {float((e3 / bound[key]).max()):.3f} of the bound")
        assert bool((e1 <= bound[key]).all()), (key, "fused", float(e1.max()), float(bound[key].max()))
        assert bool((e3 <= bound[key]).all()), (key, "three launches", float(e3.max()), float(bound[key].max()))
    assert torch.equal(xn[:B, :, :4], z.to(dtype)) and torch.equal(xn[:B], xn[B:])


@pytest.mark.parametrize("order", [2, 3])
def test_ten_step_runs_against_the_oracle(order):
    """a 10-step run with a synthetic epsilon function (no UNet): both routes against UniPCOracle in float64.  The fused route's final
    error may not exceed 2 x the three-launch route's on the same run, or the per-step parity bound summed over the steps, whichever
    is larger (it performs fewer roundings; the factor absorbs ordering differences)."""
    from imagdressing_amd import ops, scheduler as S
    from oracle.unipc import UniPCOracle
    B, HW, gs, steps = 2, 300, 7.5, 10
    W = (g(50, 4, 4) * 0.4)

    def f(z, i):          # [cond; uncond] epsilons, smooth and state-dependent; evaluated in the precision of z
        a = torch.tanh(z @ W.to(z) + 0.1 * i) + 0.05 * z
        return torch.cat([a, 0.8 * a - 0.1 * z])
    z0 = g(1, B, HW, 4)
    orc = UniPCOracle(solver_order=order)
    ts = orc.set_timesteps(steps)
    fused = S.UniPCMultistepScheduler(solver_order=order, fused_step=True, **KW)
    fused.set_timesteps(steps)
    three = S.UniPCMultistepScheduler(solver_order=order, **KW)
    three.set_timesteps(steps)
    ring = S.UniPCHistory(fused.history)
    zo, zf, zt = z0.double(), z0.clone().cuda(), z0.clone().cuda()
    H = torch.zeros(fused.history, B, HW, 4).cuda()
    budget = 0.0
    for i in range(steps):
        slots_before = list(ring.slots)                        # newest first, before this step's store
        c = ring.coefs(fused.plan_fused(i))
        # the per-step bound along the oracle's own float64 state, laid out as the kernel reads it
        Ho = torch.zeros(4, B, HW, 4, dtype=torch.float64)
        outs = [m for m in orc.model_outputs if m is not None]
        for slot, m in zip(slots_before, reversed(outs)):
            Ho[slot] = m
        if orc.last_sample is not None:
            Ho[ring.last] = orc.last_sample
        eo = f(zo, i)
        budget += float(parity_bound(zo, eo, torch.full((B,), gs), c, Ho)["z"].max())
        zo = orc.step(eo[B:] + gs * (eo[:B] - eo[B:]), ts[i], zo)
        ops.unipc_step(zf, f(zf, i).contiguous(), None, guidance=gs, coefs=c, hist=H)
        zt = three.step_guided(f(zt, i).contiguous(), zt, gs)
    torch.cuda.synchronize()
    ef, et = float((zf.cpu().double() - zo).abs().max()), float((zt.cpu().double() - zo).abs().max())
    print(f"10-step order-{order} run vs the float64 oracle: fused {ef:.3e}, three launches {et:.3e}, summed per-step bound {budget:.3e}")
    assert torch.isfinite(zf).all() and ef <= max(2.0 * et, budget), (ef, et, budget)
