"""Host side of the exact attention tests (no GPU): every case of tests/test_attention_exact_gpu.py meets the preconditions under which its
expectation is exact; the GPU file's own comparison fails, in every query row they touch, on a counted pad key, a dropped or doubled key, a causal
mask that is off by one, a second softmax added to the wrong batch entry (and, somewhere, on a first phase that was not rounded); the tolerance of
tests/test_kernels_gpu.py::test_attention lets the counted pad key pass (figures with ``-s``); an fp32 emulation of the kernels' arithmetic stays
inside the derived tolerance; every launch form and key-count residue has a case."""
import math

import pytest
import torch

from tests import attention_exact_cases as ac

F64 = torch.float64
DTS = pytest.mark.parametrize("dt", ac.DTYPES, ids=["bf16", "f16"])
SHARE = 2.0 ** -12       # a key below this share of a row's softmax moves no output by a unit in the last place of either type (11-bit significand at most, |v - o| <= 8)


# ---- preconditions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.ALL_CASES, ids=ac.case_id)
def test_cases_meet_the_preconditions(case):
    t = ac.build(case)
    assert len({c.name for c in ac.ALL_CASES}) == len(ac.ALL_CASES)
    for name in ("q", "k1", "v1") + (("k2", "v2") if case.L2 else ()):
        x = t[name]
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 256, f"{name}: integers of at most 256"
        for dt in ac.DTYPES:
            assert torch.equal(x.to(dt).to(F64), x), f"{name} changes on the way through {dt}"
    assert float(t["v1"].abs().max()) <= ac.vmax(case)
    assert t["q"].shape == (case.B, case.N, case.H, case.D) and t["k1"].shape == (-(-case.B // case.bdiv1), case.L1, case.H, case.D)
    for ph in range(2 if case.L2 else 1):
        s = ac.scores(case, ph)
        L = s.shape[-1]
        vis = ac.visible(case, L)
        assert torch.equal(s, s.round()) and float(s.abs().max()) <= 256, "scores (and with them every reference maximum) are integers of at most 256"
        hi = torch.where(vis, s, torch.full_like(s, -math.inf)).amax(-1)
        lo = torch.where(vis, s, torch.full_like(s, math.inf)).amin(-1)
        if case.family in ("count", "weighted"):
            assert float((hi - lo).max()) <= 8, "spread of a row's scores"
            # relative to the row's SMALLEST score every weight is an integer power of two: denominator and numerator are integers, exact in fp32 below 2^24
            w = torch.where(vis, torch.exp2(s - lo[..., None]), torch.zeros_like(s))
            v = t["v2" if ph else "v1"][torch.arange(case.B) // (case.bdiv2 if ph else case.bdiv1)]
            assert float(w.sum(-1).max()) < 2 ** 24 and float(torch.einsum("bhnl,blhd->bhnd", w, v.abs()).max()) < 2 ** 24
        if case.family == "count":
            assert bool((s == case.c)[..., vis].all()), "every real score is the constant c"
        if case.family == "staircase":
            want = t["q"][..., 0].permute(0, 2, 1)[..., None] * (torch.arange(L) // 64).to(F64)
            assert torch.equal(s, want) and set(t["q"][..., 0].unique().tolist()) == set(ac.STAIR_A)
    if case.family == "count" and not ac.is_causal(case) and not case.L2:
        e = ac.expectation(case, torch.bfloat16).want
        assert bool((((e - 1.0).abs() < 1e-14).sum(-1) >= 1).all()), "the 'every key' channel is 1.0 in every row"
    if case.s2 is not None:
        assert all(x == 0 or math.log2(x) == round(math.log2(x)) for x in case.s2) and len(case.s2) == case.B
        if case.split:
            assert all((x != 0) == (b < case.split) for b, x in enumerate(case.s2)), "phase2_rows = R: exactly the rows [0, R) have a second softmax"


def test_heads_and_batch_entries_differ():
    """A head or batch mix-up must change the expectation: no two (batch entry, head) slices of an expectation coincide."""
    for case in ac.ALL_CASES:
        if case.N < 8 or case.L1 < 8:
            continue
        e = ac.expectation(case, torch.float16).want
        # (count family: Q does not enter the answer, so two batch entries that SHARE their keys agree by construction)
        flat = [(b // case.bdiv1 if case.family == "count" else b, h, e[b, :, h]) for b in range(case.B) for h in range(case.H)]
        for i in range(len(flat)):
            for j in range(i):
                assert flat[i][:2] == flat[j][:2] or not torch.equal(flat[i][2], flat[j][2]), case.name


# ---- the comparison catches the mutations ---------------------------------------------------------------------------------------------------------
def applicable(case, mutation):
    if mutation == "phantom":
        return not ac.is_causal(case)               # (under the causal mask a pad key is hidden anyway: mask_gt1 is that error)
    if mutation in ("drop_boundary", "double_boundary"):
        return ac.boundary_key(case.L1) is not None
    if mutation == "mask_ge":
        return ac.is_causal(case)
    if mutation == "mask_gt1":                      # (a lone row gains nothing but the pad key: see touched_rows)
        return ac.is_causal(case) and (case.family == "count" or case.N > 1)
    if mutation == "s2_wrong_batch":
        return bool(case.L2) and tuple(torch.tensor(case.s2).roll(1).tolist()) != case.s2
    if mutation == "p1_unrounded":
        return bool(case.L2)
    return True


def _diagonal_share(case, off):
    """[B, H, N]: the share of key i + off in row i under the mask key <= query + off (off = 1: key N is a pad key, score 0)."""
    t = ac.build(case)
    s, v = ac.scores(case, 0), t["v1"]
    if off:
        s = torch.cat([s, torch.zeros(case.B, case.H, case.N, 1, dtype=F64)], -1)
        v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    vis = torch.arange(s.shape[-1])[None, :] <= torch.arange(case.N)[:, None] + off
    _, w = ac.softmax2_av(s, v[torch.arange(case.B) // case.bdiv1], vis)
    return torch.stack([w[:, :, i, i + off] for i in range(case.N)], -1)


def touched_rows(case, mutation):
    """([B, H, N] bool rows the mutation touches, [B, H, N] bool rows in which the key it concerns is visible at all).  A row is touched when the
    key holds at least SHARE of its softmax: in the count and weighted families that is every row that sees the key (asserted by the caller); on the
    staircase a key 27 or 81 base-2 units below the row's maximum is, rightly, invisible to both element types."""
    shape = (case.B, case.H, case.N)
    everything = torch.ones(shape, dtype=torch.bool)
    if mutation in ("drop_last", "drop_boundary", "double_boundary"):
        key = case.L1 - 1 if mutation == "drop_last" else ac.boundary_key(case.L1)
        return ac.key_weight(case, key) >= SHARE, ac.visible(case, case.L1)[:, key].expand(shape)
    if mutation == "mask_ge":
        return _diagonal_share(case, 0) >= SHARE, everything
    if mutation == "mask_gt1":
        rows = _diagonal_share(case, 1) >= SHARE
        if case.family != "count":          # row N - 1 gains a pad key (score 0, V = 0), i.e. the phantom key: the count family's to catch (see below)
            rows[..., -1] = False
            everything = everything.clone()
            everything[..., -1] = False
        return rows, everything
    if mutation == "s2_wrong_batch":
        s2 = torch.tensor(case.s2)
        rows = (s2 != s2.roll(1))[:, None, None].expand(shape)
        return rows, rows
    return everything, everything


@pytest.mark.parametrize("case", ac.ALL_CASES, ids=ac.case_id)
@DTS
def test_the_comparison_fails_on_every_row_a_mutation_touches(case, dt):
    exp = ac.expectation(case, dt)
    assert not bool(ac.mismatches(exp.want, exp).any()) and not bool(ac.mismatches(ac.round_dt(exp.want, dt), exp).any())
    if case.family == "count":          # elements held to equality: both types can hold them; one key set: the "every key" channel of every row is among them
        assert torch.equal(ac.round_dt(exp.want, dt)[exp.exact], exp.want[exp.exact]) and (bool(case.L2) or bool(exp.exact.any(-1).all()))
    for mutation in ac.MUTATIONS:
        if not applicable(case, mutation) or mutation == "p1_unrounded":
            continue
        if mutation == "phantom" and not (case.family == "count" and case.c == -8):
            continue        # one pad key among L real ones at the same score is 1 / L of the denominator: below bf16's resolution from L of a few hundred on;
                            # at c = -8 it weighs 2^8 keys (test_a_counted_pad_key_... below)
        wrong = ac.round_dt(ac.expectation(case, dt, mutation).want, dt)          # what a kernel with that error would store
        bad = ac.mismatches(wrong, exp).any(-1).permute(0, 2, 1)          # [B, H, N]
        rows, seen = touched_rows(case, mutation)
        if case.family != "staircase":
            assert torch.equal(rows, seen), f"{case.name}: {mutation} should touch every row that sees the key"
        assert int(rows.sum()) > 0, f"{case.name}: {mutation} touches nothing"
        missed = rows & ~bad
        assert not bool(missed.any()), (f"{case.name} [{ac.DT_NAME[dt]}] {mutation}: passes the comparison in {int(missed.sum())} of {int(rows.sum())} touched rows, "
                                        f"first (batch, head, row) {missed.nonzero()[0].tolist()}")
        with pytest.raises(AssertionError, match="query row"):
            ac.assert_exact(wrong, exp, case.name)


@DTS
def test_a_counted_pad_key_is_caught_at_every_key_count(dt):
    """c = -8: a counted pad key (score 0) weighs 2^8 real keys, so every row fails at every L, in bf16 too; c = 0 alone misses it in bf16 once 1 / L
    drops below the type's resolution.  Every non-causal launch form and key count of the GPU file has such a case."""
    for form, cases in (("generic", ac.GENERIC_CASES), ("d40", ac.D40_CASES)):
        have = {(c.D, c.L1) for c in cases if c.family == "count" and c.c == -8}
        assert have >= {(c.D, c.L1) for c in cases}, form
    missed_at_zero = 0
    for L in (65, 127, 289, 640, 1345):
        for c in (-8, 0):
            case = ac._case("generic", "count", 40, 2, 2, 33, L, c=c)
            exp = ac.expectation(case, dt)
            bad = ac.mismatches(ac.round_dt(ac.expectation(case, dt, "phantom").want, dt), exp).any(-1)
            print(f"{ac.DT_NAME[dt]} L={L} c={c}: rows caught {int(bad.sum())}/{bad.numel()}")
            if c == -8:
                assert bool(bad.all()), f"L={L}"
            else:
                missed_at_zero += int((~bad).sum())
    assert (missed_at_zero > 0) == (dt == torch.bfloat16)


@DTS
def test_an_unrounded_first_phase_is_caught_somewhere(dt):
    """want = round_dt(p1) + s2 p2: a kernel that adds the UNROUNDED first phase is off by at most ulp(p1) / 2, visible where the sum is much smaller
    than p1 (weighted family: opposite signs)."""
    caught = {}
    for case in ac.ALL_CASES:
        if applicable(case, "p1_unrounded"):
            exp = ac.expectation(case, dt)
            caught[case.name] = int(ac.mismatches(ac.round_dt(ac.expectation(case, dt, "p1_unrounded").want, dt), exp).sum())
    hit = {k: v for k, v in caught.items() if v}
    print(f"{ac.DT_NAME[dt]}: caught in {len(hit)} of {len(caught)} two-phase cases, {sum(hit.values())} elements")
    assert len(hit) >= 1


# ---- what the older comparison lets through ---------------------------------------------------------------------------------------------------------
OLD_SHAPES = [(40, 2, 200, 200, 330), (40, 1, 1100, 1100, 0), (80, 2, 144, 144, 100), (160, 1, 64, 64, 80), (64, 2, 16, 273, 0), (40, 2, 130, 77, 4),
              (160, 1, 70, 77, 0)]          # the parameters of tests/test_kernels_gpu.py::test_attention


@pytest.mark.parametrize("D,B,N,L1,L2", OLD_SHAPES)
@DTS
def test_the_gaussian_comparison_accepts_a_counted_pad_key(D, B, N, L1, L2, dt):
    """test_attention's inputs, reference and tolerance (atol = rtol = 1e-2), with ONE pad key (K = 0, V = 0: score 0) counted in the first softmax's
    denominator: accepted at every shape in both types -- why the exact tests exist."""
    from tests.test_kernels_gpu import assert_close, ref_attn, rnd
    H = 8
    Cc = H * D
    q = rnd(1, B, N, Cc).to(dt); k1 = rnd(2, B, L1, Cc).to(dt); v1 = rnd(3, B, L1, Cc).to(dt)
    ref = ref_attn(q, k1, v1, H)
    sc = D ** -0.5 * math.log2(math.e)
    s = torch.einsum("bnhd,blhd->bhnl", q.to(F64).view(B, N, H, D), k1.to(F64).view(B, L1, H, D)) * sc
    wrong, _ = ac.softmax2_av(s, v1.to(F64).view(B, L1, H, D), torch.ones(N, L1, dtype=torch.bool), phantom=1)
    wrong = wrong.reshape(B, N, Cc)
    if L2:
        k2 = rnd(4, 1, L2, Cc).to(dt); v2 = rnd(5, 1, L2, Cc).to(dt)
        s2 = torch.tensor([0.9, 0.0][:B] if B == 2 else [0.9])
        r2 = ref_attn(q, k2.expand(B, -1, -1), v2.expand(B, -1, -1), H)
        ref = ref.to(dt).float() + s2[:, None, None] * r2
        wrong = wrong.to(dt).to(F64) + s2[:, None, None].to(F64) * r2.to(F64)
    got = wrong.to(dt)
    err = (got.float() - ref.float()).abs()
    print(f"D={D} B={B} N={N} L1={L1} L2={L2} {ac.DT_NAME[dt]}: largest error of the mutated output {err.max().item():.3g}, output std {ref.float().std().item():.3g}, "
          f"elements outside atol = rtol = 1e-2: {int((err > 1e-2 + 1e-2 * ref.float().abs()).sum())}")
    assert_close(got, ref, atol=1e-2, rtol=1e-2, what=f"attention D={D}")


# ---- the tolerance derivation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.ALL_CASES, ids=ac.case_id)
@DTS
def test_an_fp32_emulation_of_the_kernels_stays_inside_the_tolerance(case, dt):
    """32-key blocks, fp32 accumulators, P rounded to the element type, o * (1 / l): with the deferred maximum (threshold 8), with the exact running
    maximum, and -- head dim 40 -- with variant 13's unchecked steps (fp16: first maximum + 4; a denominator that leaves fp32 runs again checked)."""
    exp = ac.expectation(case, dt)
    modes = [(8.0, 0.0, False), (0.0, 0.0, False)]
    if case.D == 40 and not ac.is_causal(case):
        modes.append((8.0, 4.0 if dt == torch.float16 else 0.0, True))
    for thr, bias, unchecked in modes:
        ac.assert_exact(ac.emulate(case, dt, thr, bias, unchecked), exp, f"emulation (threshold {thr}, bias {bias}, unchecked {unchecked}) of {case.name}")


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------------------
def _units(L):
    n = -(-L // 64)
    return 1 if n == 1 else 2 if n == 2 else 4 if n >= 4 else 3


def test_every_launch_form_and_key_count_has_a_case():
    assert {L % 64 for L in ac.LS} >= set(ac.RESIDUES) and {_units(L) for L in ac.LS} >= {1, 2, 4}
    assert {L % 64 for L in ac.LS if 1 <= L % 64 <= 32} and {L for L in ac.LS if L < 32}        # a whole 32-key block past the end; fewer keys than one block
    g = ac.GENERIC_CASES
    for D in (40, 64, 80, 160):
        mine = [c for c in g if c.D == D]
        assert {c.L1 for c in mine} == set(ac.LS) and {c.family for c in mine} == {"count", "weighted"} and {c.c for c in mine} == {0, -8}
        assert {c.N % 128 == 0 for c in mine} == {True, False} and len({c.N for c in mine}) >= 4 and all(c.N < 512 for c in mine)
        assert any(c.bdiv1 > 1 for c in mine) and any(c.L2 and c.bdiv2 > 1 for c in mine) and any(c.L2 and c.bdiv2 == 1 for c in mine)
        assert {c.L2 % 64 for c in mine if c.L2} >= set(ac.RESIDUES)
        assert all(bool(c.split) == (D != 40) for c in mine if c.L2) and {c.B for c in mine} == {2, 3} and {c.H for c in mine} == {2, 3}
        assert len({c.split for c in mine if c.L2}) == (2 if D != 40 else 1)
    cz = ac.CAUSAL_CASES
    assert {(c.D, c.N) for c in cz} == {(D, N) for D in (64, 80, 40) for N in (1, 33, 64, 77, 130)} and all(c.N == c.L1 and not c.L2 for c in cz)
    for D in (64, 80, 40):
        assert {(c.family, c.c) for c in cz if c.D == D} == {("count", 0), ("count", -8), ("weighted", 0)}
    d = ac.D40_CASES
    assert {c.N for c in d} == {512, 530} and {c.L1 for c in d} == set(ac.LS) | {ac.L_LONG}
    assert all(set(c.variants) == set(range(1, 14)) and set(c.pad_one) == {True, False} and c.D == 40 and c.B == 2 for c in d)
    assert any(c.L2 and c.s2 == (1.0, 0.0) for c in d) and any(c.L2 and c.s2[0] == 0 and c.s2[1] != 0 for c in d) and any(not c.L2 for c in d)
    assert {c.L2 % 64 for c in d if c.L2} >= {0, 1, 31, 33} and any(c.L1 == ac.L_LONG and c.L2 for c in d)
    st = ac.STAIRCASE_CASES
    assert {(c.D, c.N < 512) for c in st} == {(40, True), (80, True), (40, False)} and all(c.L1 == 640 for c in st)
    assert [set(c.variants) for c in st if c.N >= 512] == [{12, 13}]
