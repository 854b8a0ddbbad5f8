"""Host side of the exact attention tests at head dim 512 (no GPU), as tests/test_attention_exact_inputs.py is for the other head dims: every
case of tests/attention_d512_cases.py meets the preconditions under which its expectation is exact; an fp32 emulation of the kernel's arithmetic
(32-key tiles, exact running maximum -- and the deferred one, which the kernel is free to use) stays inside the derived tolerance; the GPU file's
comparison fails in EVERY (batch entry, head, query row) on a counted pad key and on a dropped last key, at 16449 keys too.  And the library --
which loads without a GPU -- answers imd_attn_padded_dims(512) with (512, 512)."""
import pytest
import torch

from tests import attention_d512_cases as dc
from tests import attention_exact_cases as ac

F64 = torch.float64
DTS = pytest.mark.parametrize("dt", ac.DTYPES, ids=["bf16", "f16"])
CASES = pytest.mark.parametrize("case", dc.CASES, ids=ac.case_id)


def test_the_case_list_is_what_the_kernel_needs():
    cs = dc.CASES
    assert len({c.name for c in cs}) == len(cs) and all(c.D == 512 and not c.L2 and not ac.is_causal(c) for c in cs)
    short = [c for c in cs if c.family != "staircase" and c.L1 != dc.LIMIT_L]
    assert {c.L1 for c in short} == set(ac.LS) | {ac.L_LONG} and {c.N for c in short} == set(ac.GENERIC_N)
    for L in ac.LS + (ac.L_LONG,):
        assert {(c.family, c.c) for c in short if c.L1 == L} == set(ac.FAMILIES)
    assert {(c.B, c.H) for c in short} == {(3, 1), (2, 2)} and {c.bdiv1 for c in short} == {1, 2}
    assert [(c.N, c.L1) for c in cs if c.family == "staircase"] == [(130, 640)]
    past = [c for c in cs if c.L1 == dc.LIMIT_L]
    assert [(c.family, c.c, c.B, c.H, c.N) for c in past] == [("count", -8, 1, 1, 70), ("count", 0, 1, 1, 70), ("weighted", 0, 1, 1, 70)]
    assert dc.LIMIT_L > 16384 and dc.LIMIT_L % 32 == 1


@CASES
def test_cases_meet_the_preconditions(case):
    t = ac.build(case)
    for name in ("q", "k1", "v1"):
        x = t[name]
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 256, f"{name}: integers of at most 256"
        for dt in ac.DTYPES:
            assert torch.equal(x.to(dt).to(F64), x), f"{name} changes on the way through {dt}"
    assert float(t["v1"].abs().max()) <= ac.vmax(case)
    assert t["q"].shape == (case.B, case.N, case.H, case.D) and t["k1"].shape == (-(-case.B // case.bdiv1), case.L1, case.H, case.D)
    s = ac.scores(case, 0)
    assert torch.equal(s, s.round()) and float(s.abs().max()) <= 256, "scores (and with them every running maximum) are integers of at most 256"
    if case.family in ("count", "weighted"):
        hi, lo = s.amax(-1), s.amin(-1)
        assert float((hi - lo).max()) <= 8, "spread of a row's scores"
        # relative to the row's SMALLEST score every weight is an integer power of two: denominator and numerator are integers, exact in fp32 below 2^24
        w = torch.exp2(s - lo[..., None])
        v = t["v1"][torch.arange(case.B) // case.bdiv1]
        assert float(w.sum(-1).max()) < 2 ** 24 and float(torch.einsum("bhnl,blhd->bhnd", w, v.abs()).max()) < 2 ** 24
    if case.family == "count":
        assert bool((s == case.c).all()), "every real score is the constant c"
        e = ac.expectation(case, torch.bfloat16).want
        assert bool((((e - 1.0).abs() < 1e-14).sum(-1) >= 1).all()), "the 'every key' channel is 1.0 in every row"
    if case.family == "staircase":
        want = t["q"][..., 0].permute(0, 2, 1)[..., None] * (torch.arange(case.L1) // 64).to(F64)
        assert torch.equal(s, want) and set(t["q"][..., 0].unique().tolist()) == set(ac.STAIR_A)


@CASES
@DTS
def test_an_fp32_emulation_of_the_kernel_stays_inside_the_tolerance(case, dt):
    """32-key tiles, fp32 accumulators, P rounded to the element type, o * (1 / l): with the exact running maximum (what attention_d512.hip does) and
    with the deferred one (threshold 8), which it may use."""
    exp = ac.expectation(case, dt)
    for thr in (8.0, 0.0):
        got = ac.emulate(case, dt, thr)
        ac.assert_exact(got, exp, f"emulation (threshold {thr}) of {case.name}")


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.family != "staircase"], ids=ac.case_id)
@DTS
def test_the_comparison_fails_in_every_row_on_a_counted_pad_key_and_on_a_dropped_key(case, dt):
    """phantom: one pad key (K = 0, V = 0: score 0) counted -- count family at c = -8, where it weighs 2^8 real keys (at c = 0 it is 1 / L of the
    denominator, below bf16's resolution from a few hundred keys on: tests/test_attention_exact_inputs.py).  drop_last: key L - 1 lost -- count
    (both c) and weighted."""
    exp = ac.expectation(case, dt)
    assert not bool(ac.mismatches(exp.want, exp).any()) and not bool(ac.mismatches(ac.round_dt(exp.want, dt), exp).any())
    mutations = ["drop_last"] + (["phantom"] if case.family == "count" and case.c == -8 else [])
    for mutation in mutations:
        wrong = ac.round_dt(ac.expectation(case, dt, mutation).want, dt)          # what a kernel with that error would store
        bad = ac.mismatches(wrong, exp).any(-1)                                   # [B, N, H]
        assert bool(bad.all()), f"{case.name} [{ac.DT_NAME[dt]}] {mutation}: passes the comparison in {int((~bad).sum())} of {bad.numel()} (batch, row, head) rows"
        with pytest.raises(AssertionError, match="query row"):
            ac.assert_exact(wrong, exp, case.name)


def test_the_library_answers_padded_dims_512():
    """Loads the built library (no GPU needed): head dim 512 has no pad columns."""
    import ctypes as C

    from imagdressing_amd import _lib
    lib = _lib.load()
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.imd_attn_padded_dims(512, C.byref(a), C.byref(b)) == 0, "imd_attn_padded_dims(512) is refused"
    assert (a.value, b.value) == (512, 512) == ac.padded_dims(512)
