"""Host-side checks of tests/layernorm_cases.py, the harness of tests/test_layernorm_exact_gpu.py: every case meets its preconditions, the fp32
emulation of a CORRECT kernel passes every bar (the reference alone stays within them), every mutant is rejected, and the stored constants are
what the emulation yields.  No GPU, nothing of the package.

Which regime rejects which mutant (layernorm_cases.MUTANT_CAUGHT_BY, asserted for K in {320, 640, 1280} x {bf16, fp16}):
  eps swapped, eps = 0                             eps_dominated at both eps
  variance / (K - 1)                               the scale statistic on ``general`` (in bf16 nothing else sees it)
  mean of the first half                           general
  squared deviations of the second half dropped    general, eps_dominated
  one-pass variance in fp32                        large_mean: r = 128 in fp16, r = 388 on bf16's own grid
  one channel left out of both sums                outlier (the 200 of row 0 sits on the last channel), large_mean r = 32
  rstd of the neighbouring row                     general (neighbouring rows differ by a factor of two)"""
import pytest
import torch

from tests import exact_cases as ec
from tests import layernorm_cases as lc

F64 = torch.float64
DTS = pytest.mark.parametrize("dt", lc.DTYPES, ids=[lc.DT_NAME[d] for d in lc.DTYPES])
KS = pytest.mark.parametrize("K", lc.KS)


@pytest.mark.parametrize("C", lc.ALL_C)
@DTS
def test_values_are_exact_in_the_element_type(C, dt):
    for case in lc.family_cases(C, dt):
        assert case.x.dtype == F64 and case.x.shape[1] == C
        assert torch.equal(lc.round_dt(case.x, dt), case.x), case.name
        assert bool(torch.isfinite(case.x).all())
    assert lc.general(C, dt).shape[0] == lc.GENERAL_ROWS >= 256
    assert max(lc.SCALE_ROWS[C]) <= lc.GENERAL_ROWS


@pytest.mark.parametrize("C", lc.ALL_C)
def test_eps_dominated_statistics_are_exact(C):
    x = lc.eps_dominated(C)
    assert torch.equal(x.abs(), torch.full_like(x, 2.0 ** -9)) and torch.equal((x > 0).sum(1), torch.full((x.shape[0],), C // 2))
    assert not torch.equal(x[0], x[1])                                    # the signs are permuted per row
    assert torch.equal(x.sum(1), torch.zeros(x.shape[0], dtype=F64))
    assert torch.equal((x * x).sum(1) / C, torch.full((x.shape[0],), 2.0 ** -18, dtype=F64))
    # ... and in fp32, in sequential order: every partial sum is a small multiple of 2^-9 / 2^-18
    x32 = x.float()
    assert torch.equal(lc._seq_sum32(x32.unbind(-1)), torch.zeros(x.shape[0]))
    assert torch.equal(lc._seq_sum32((x32 * x32).unbind(-1)) / C, torch.full((x.shape[0],), 2.0 ** -18))
    for eps in lc.EPS_VALUES:                                             # |n| = 0.5255 / 0.8901
        assert float((lc.reference(x, eps).abs() - 2.0 ** -9 / (2.0 ** -18 + eps) ** 0.5).abs().max()) < 1e-12


@KS
@DTS
def test_large_mean_has_the_ratio_it_claims(K, dt):
    for r in lc.LARGE_MEAN_R[dt]:
        x = lc.large_mean(K, dt, r)
        mean = x.mean(1)
        var = ((x - mean[:, None]) ** 2).mean(1)
        # over the case (64 K elements); a single row of 320 samples estimates its std to 4 % only, so the rows spread to 10 % by themselves
        ratio = float(mean.abs().mean() / var.mean().sqrt())
        assert abs(ratio / r - 1) < 0.1, f"r={r}: |mean| / std = {ratio:.1f}"
        assert float(((mean.abs() / var.sqrt()) / r - 1).abs().max()) < 0.2
        assert bool((mean[0::2] > 0).all()) and bool((mean[1::2] < 0).all())


@KS
@DTS
def test_general_and_outlier_are_what_they_claim(K, dt):
    x = lc.general(K, dt)
    rms = (x - x.mean(1, keepdim=True)).pow(2).mean(1).sqrt()
    j = (torch.arange(lc.GENERAL_ROWS) % 13 - 6).to(F64)
    assert float((torch.log2(rms / 1.6) - j).abs().max()) < 0.25          # std sqrt(1.5^2 + 0.6^2) = 1.6, times 2^j
    assert float(rms.min()) ** 2 > 10 * 1e-5                              # away from eps at every scale
    o = lc.outlier(K, dt)
    n = lc.reference(o, 1e-5)
    assert torch.equal(o.max(1).values, torch.full((16,), 200.0, dtype=F64)) and int(o[0].argmax()) == K - 1
    assert float((n.max(1).values / K ** 0.5 - 1).abs().max()) < 0.05


@pytest.mark.parametrize("form", lc.FORMS)
@KS
@DTS
def test_emulation_of_a_correct_kernel_passes_every_bar(K, dt, form):
    assert lc.run_checks(lambda x, eps: lc.emulate(x, eps, form), K, dt) == []
    x = lc.general(K, dt)
    y = lc.reference(x, 1e-5)
    _, worst, _, _ = lc.element_bar(lc.round_dt(lc.emulate(x, 1e-5, form), dt), y, dt, lc.A_ABS)
    print(f"K={K} {lc.DT_NAME[dt]} {form}: worst element error on general {worst:.3f} ulp")
    assert worst <= 0.6                                                   # half an ulp, plus the fp32 noise on elements near zero


@pytest.mark.parametrize("C", lc.S1_CS)
@DTS
def test_emulation_with_an_affine_passes_every_bar(C, dt):
    """ops.layer_norm's form at its own widths: fp32 (x - mean) rstd gamma + beta against affine_expectation."""
    gamma, beta = ec.away_from_zero_affine(11, C)
    for case in lc.family_cases(C, dt):
        y, A = lc.affine_expectation(case, gamma, beta)
        n32 = lc.emulate(case.x, case.eps, "div").float()
        got = lc.round_dt((n32 * gamma + beta).to(F64), dt)
        ok, worst, _, bad = lc.element_bar(got, y, dt, A)
        assert ok, f"C={C} {case.name}: {bad} elements beyond the bar, worst {worst:.3f} ulp"
    for rows in lc.SCALE_ROWS[C][:1]:
        x = lc.general(C, dt)[:rows]
        y = lc.reference(x, 1e-5)
        assert abs(lc.scale_statistic(lc.round_dt(lc.emulate(x, 1e-5, "div"), dt), y) - 1) <= lc.scale_bound(C, dt, rows)


@pytest.mark.parametrize("name", list(lc.MUTANTS))
@KS
@DTS
def test_every_mutant_is_rejected(K, dt, name):
    failed = lc.run_checks(lc.MUTANTS[name], K, dt)
    print(f"K={K} {lc.DT_NAME[dt]} {name}: rejected by {failed}")
    assert failed, "no check rejects this mutant"
    missing = [c for c in lc.MUTANT_CAUGHT_BY[name][dt] if c not in failed]
    assert not missing, f"expected {missing} to reject it as well; rejected by {failed}"


@KS
@DTS
def test_scale_error_is_beyond_the_scale_bound(K, dt):
    """1 / (2 K) against the bound, with room: the statistic, not luck, rejects the K - 1 variance."""
    for rows in lc.SCALE_ROWS[K]:
        assert lc.scale_bound(K, dt, rows) < 0.25 / (2 * K)


def test_s6_bar_equals_the_issue_form_away_from_binade_edges():
    """ff_expectation's ulp term is ulp(n64) + ulp(x + n64) / 2 except within ulp(n64) of a power of two (there: the next binade's)."""
    for dt in lc.DTYPES:
        case = lc.family_cases(320, dt)[0]
        want, ulp = lc.ff_expectation(case, 300, dt)
        n = lc.reference(case.x, case.eps)
        plain = ec.ulp_at(n, dt) + ec.ulp_at(want, dt) / 2
        assert bool((ulp >= plain).all()) and float((ulp != plain).double().mean()) < 0.02


@DTS
def test_feed_forward_site_bars(dt):
    """round_dt(x + round_dt(emulation)) passes S6's bar in every case and its scale statistic; with the K - 1 variance the statistic rejects it."""
    for M in (1, 300):
        for case in lc.family_cases(320, dt):
            want, ulp = lc.ff_expectation(case, M, dt)
            x = lc.take_rows(case.x, M)
            got = lc.round_dt(x + lc.round_dt(lc.emulate(x, case.eps, "fused"), dt), dt)
            ok, worst, _, bad = lc.element_bar(got, want, dt, lc.abs_term(case), ulp)
            assert ok, f"{case.name}: {bad} elements beyond the bar, worst {worst:.3f}"
    x = lc.general(320, dt)
    s_err, bound = lc.ff_scale(lc.round_dt(x + lc.round_dt(lc.emulate(x, 1e-5, "fused"), dt), dt), dt)
    assert s_err <= bound
    s_bad, _ = lc.ff_scale(lc.round_dt(x + lc.round_dt(lc.MUTANTS["variance / (K - 1)"](x, 1e-5), dt), dt), dt)
    assert s_bad > 4 * bound
    assert lc.ff_scale_ideal(dt) == pytest.approx(lc.FF_SCALE_IDEAL[lc.DT_NAME[dt]], rel=1e-6)


def test_stored_constants_are_what_the_emulation_yields():
    want_a = {(C, lc.DT_NAME[dt], r) for C in lc.ALL_C for dt in lc.DTYPES for r in lc.LARGE_MEAN_R[dt]}
    assert set(lc.LARGE_MEAN_A) == want_a
    for C in lc.ALL_C:
        for dt in lc.DTYPES:
            for r in lc.LARGE_MEAN_R[dt]:
                stored = lc.LARGE_MEAN_A[(C, lc.DT_NAME[dt], r)]
                assert lc.large_mean_a(C, dt, r) == pytest.approx(stored, rel=1e-6), (C, dt, r)
                assert 1e-7 < stored < 2e-4
            for rows in lc.SCALE_ROWS[C]:
                assert lc.scale_ideal(C, dt, rows) == pytest.approx(lc.SCALE_IDEAL[(C, lc.DT_NAME[dt], rows)], rel=1e-6, abs=1e-12), (C, dt, rows)
    assert set(lc.SCALE_IDEAL) == {(C, lc.DT_NAME[dt], rows) for C in lc.ALL_C for dt in lc.DTYPES for rows in lc.SCALE_ROWS[C]}
