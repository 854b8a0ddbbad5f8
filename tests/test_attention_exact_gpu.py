"""imd_attention on integer-valued heads, where softmax2(S) V is known to the last place (tests/attention_exact_cases.py; preconditions, the
sensitivity of the comparison and the fp32 emulation behind the tolerance: tests/test_attention_exact_inputs.py).

Every launch form of attention.hip and attention_d40.hip: the generic kernel at head dims 40 (N < 512) / 64 / 80 / 160 with ragged and whole
row blocks, shared K / V (kv_bdiv > 1), a second key set with its own ragged tail, the phase-split launch against the one-workgroup form
(bit for bit); the causal mask at head dims 64 / 80 / 40; every head-dim-40 variant imd_set_tuning(0, .) accepts (1..5: the generic kernel's
other template forms, 6..13: the pipelined kernel with and without the caller's K pad column) with a second key set on one of two batch rows
and with out_dup; scores that climb or fall by whole 64-key units (deferred-maximum raises, unchecked growth, the fp16 re-run).  Key counts:
L % 64 in {0, 1, 31, 32, 33, 63} at one, two and five 64-key units, and 1345 keys for the ring of three.

The comparison is one unit in the last place of the element type (the bound is derived in tests/attention_exact_cases.py): a pad key that
is counted, a dropped or doubled key, a mask that is off by one, a second softmax added to the wrong batch entry all fail it in every row.

Guards: `out` is a window of a sentinel-filled buffer with out_ld = H D + 8 and two rows in front of the first and behind the last batch
entry (imd_attn_params.out has no batch stride: row N of entry b IS row 0 of entry b + 1); nothing outside [rows, H D) may change."""
import contextlib

import pytest
import torch

from tests import attention_exact_cases as ac

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
SENTINEL = -976.0            # representable in both types, far outside every expectation (|want| <= 12), finite
GUARD_ROWS, GUARD_COLS = 2, 8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def upload(case, dt, pad_one):
    return {k: (None if v is None else v.to("cuda")) for k, v in ac.pack(case, dt, pad_one).items()}


def launch(ops, case, dt, d, *, pad_one=False, variant=None, split=0, dup=False):
    """One imd_attention launch into guarded buffers; returns the whole buffers (out, out_dup or None) on the CPU."""
    rows, ld = case.B * case.N, case.H * case.D + GUARD_COLS
    full = torch.full((rows + 2 * GUARD_ROWS, ld), SENTINEL, dtype=dt, device="cuda")
    dfull = torch.full_like(full, SENTINEL) if dup else None
    kw = dict(B=case.B, H=case.H, N=case.N, D=case.D, L1=case.L1, L1P=ac.pad64(case.L1), kv1_bdiv=case.bdiv1, out_ld=ld,
              causal=ac.is_causal(case), k_pad_one=pad_one)
    if case.L2:
        kw.update(k2=d["k2"], v2t=d["v2t"], scale2=torch.tensor(case.s2, dtype=torch.float32, device="cuda"), L2=case.L2, L2P=ac.pad64(case.L2),
                  kv2_bdiv=case.bdiv2)
    if split:
        assert ops.ATTN_PHASE_SPLIT and ops.attention_phase_split_supported(case.D) and case.N <= ops.ATTN_PHASE_SPLIT_MAX_N
        kw["phase2_rows"] = split
    if dup:
        assert ops.attention_dup_supported(case.H, case.N, case.D)
        kw["out_dup"] = dfull[GUARD_ROWS:GUARD_ROWS + rows]
    with (ops.tuning_scope(attn_variant=variant) if variant else contextlib.nullcontext()):
        ops.attention(d["q"], d["k1"], d["v1t"], full[GUARD_ROWS:GUARD_ROWS + rows], **kw)
    torch.cuda.synchronize()
    return full.cpu(), (None if dfull is None else dfull.cpu())


def check(full, case, exp, what):
    rows, C = case.B * case.N, case.H * case.D
    bits = full.view(torch.int16)
    fresh = torch.full((1,), SENTINEL, dtype=full.dtype).view(torch.int16).item()
    assert bool((bits[:GUARD_ROWS] == fresh).all()), f"{what}: rows in front of the first batch entry were written"
    assert bool((bits[GUARD_ROWS + rows:] == fresh).all()), f"{what}: rows behind query row N - 1 of the last batch entry were written"
    assert bool((bits[:, C:] == fresh).all()), f"{what}: columns at or beyond H * D = {C} were written"
    got = full[GUARD_ROWS:GUARD_ROWS + rows, :C]
    assert bool(torch.isfinite(got.float()).all()), f"{what}: {int((~torch.isfinite(got.float())).sum())} written elements are not finite"
    ac.assert_exact(got, exp, what)
    return got


def test_padded_dims_match_the_library(ops):
    for D in (40, 64, 80, 160):
        assert ops.attn_padded_dims(D) == ac.padded_dims(D)
        assert bool(ops.attention_phase_split_supported(D)) == (D != 40)


@pytest.mark.parametrize("case", ac.GENERIC_CASES, ids=ac.case_id)
@DTS
def test_generic_kernel(ops, case, dt):
    """attention.hip at every head dim: ragged and whole 128-row blocks, shared K / V, a second key set, the phase-split launch."""
    exp = ac.expectation(case, dt)
    d = upload(case, dt, False)
    plain = None
    for variant in case.variants or (None,):
        full, _ = launch(ops, case, dt, d, variant=variant)
        got = check(full, case, exp, f"{case.name} variant {variant}")
        plain = got if plain is None else plain
    if case.split:
        full, _ = launch(ops, case, dt, d, split=case.split)
        got = check(full, case, exp, f"{case.name} phase-split (rows {case.split})")
        assert torch.equal(got.view(torch.int16), plain.view(torch.int16)), f"{case.name}: the phase-split launch differs from the one-workgroup form"


@pytest.mark.parametrize("case", ac.CAUSAL_CASES, ids=ac.case_id)
@DTS
def test_causal_mask(ops, case, dt):
    """The causal form (CLIP's towers run it at head dims 64 / 80, N = 77): count family -- row i gives exactly 1.0 in the "every key" channel and
    1 / (i + 1) per visible single key; weighted family likewise to the last place."""
    exp = ac.expectation(case, dt)
    full, _ = launch(ops, case, dt, upload(case, dt, False))
    check(full, case, exp, case.name)


@pytest.mark.parametrize("case", ac.D40_CASES, ids=ac.case_id)
@DTS
def test_d40_variants(ops, case, dt):
    """N >= 512 at head dim 40: variants 1..5 (attention.hip's other template forms) and 6..13 (attention_d40.hip), with and without the caller's
    K pad column; then out_dup (variants 12 / 13): `out` as before, `out_dup` the first phase alone of EVERY batch entry."""
    exp = ac.expectation(case, dt)
    for pad_one in case.pad_one:
        d = upload(case, dt, pad_one)
        for variant in case.variants:
            full, _ = launch(ops, case, dt, d, pad_one=pad_one, variant=variant)
            check(full, case, exp, f"{case.name} variant {variant} k_pad_one={int(pad_one)}")
        if pad_one:
            first = ac.first_phase(case, dt)
            for variant in ac.D40_DUP_VARIANTS:
                full, dfull = launch(ops, case, dt, d, pad_one=True, variant=variant, dup=True)
                check(full, case, exp, f"{case.name} variant {variant} with out_dup: out")
                check(dfull, case, first, f"{case.name} variant {variant}: out_dup")


@pytest.mark.parametrize("case", ac.STAIRCASE_CASES, ids=ac.case_id)
@DTS
def test_staircase_scores(ops, case, dt):
    """Scores a_i floor(j / 64) over ten 64-key units: rows with +9 raise the deferred maximum at every unit, rows with +3 grow P unchecked in
    variant 13 (fp16: overflow and the re-run as variant 12), rows with -3 never raise; every P, maximum and rescale stays a power of two."""
    exp = ac.expectation(case, dt)
    for pad_one in case.pad_one:
        d = upload(case, dt, pad_one)
        for variant in case.variants or (None,):
            full, _ = launch(ops, case, dt, d, pad_one=pad_one, variant=variant)
            check(full, case, exp, f"{case.name} variant {variant} k_pad_one={int(pad_one)}")
