"""The exact cases of guidance_rescale_cases.py without a GPU: their preconditions hold at every size the GPU test uses (build()
asserts them in float64), each fault a row-reduction kernel can have changes the expected tensor there, and the float64 oracle equals
a literal torch.std restatement of diffusers' rescale_noise_cfg."""
import pytest
import torch

from tests import guidance_rescale_cases as cases
from tests.guidance_rescale_oracle import factors, guidance_rescale, rescale_noise_cfg_literal


@pytest.mark.parametrize("HW", cases.HW_SIZES)
def test_families_are_exact_and_see_every_fault(HW):
    for g in cases.GS:
        for phi in cases.PHIS:
            eps, want = cases.build("A", HW, g, phi)
            assert torch.equal(want[0], (phi + g * (1 - phi)) * eps[0]) and torch.equal(want[1], want[0])
            # (u = 0 makes e proportional to t: a reduction that loses or repeats an element of BOTH keeps the ratio -- family B sees it)
            assert not torch.equal(cases.faulty(eps, g, phi, "cond_only"), want.double()), (HW, g, phi)
    for phi in cases.PHIS:
        eps, want = cases.build("B", HW, 8.0, phi)
        assert torch.equal(want[0], (phi / 8 + 1 - phi) * (64 + 8 * (eps[0] - 64)))
        for fault in ("drop", "double", "uncentred", "cond_only"):
            assert not torch.equal(cases.faulty(eps, 8.0, phi, fault), want.double()), (fault, HW, phi)
        for phi_c in (phi, 0.7):
            eps, want = cases.build("C", HW, 8.0, phi_c)
            assert torch.equal(want, eps)
    # per row: g and phi differ between the rows, so the statistics of the neighbouring row give another factor
    g3, p3 = [2.0, 4.0, 8.0], [1.0, 0.5, 0.25]
    for fam, faults in (("A", ("neighbour", "cond_only")), ("B", ("neighbour", "drop", "double", "uncentred", "cond_only"))):
        eps, want = cases.build(fam, HW, g3, p3, B=3)
        for fault in faults:
            assert not torch.equal(cases.faulty(eps, g3, p3, fault), want.double()), (fam, fault, HW)
    # the faultless restatement IS the oracle
    assert torch.equal(cases.faulty(eps, g3, p3, None), want.double())


def test_cond_only_write_shows_in_a_step_with_guidance():
    """e' in the cond half only: a step that computes u + g (c - u) with g != 1 then differs from e'"""
    eps, want = cases.build("A", 65, 4.0, 0.5)
    bad = cases.faulty(eps, 4.0, 0.5, "cond_only")
    g = 4.0
    assert torch.equal(want[1].double() + g * (want[0].double() - want[1].double()), want[0].double())
    assert not torch.equal(bad[1] + g * (bad[0] - bad[1]), want[0].double())


def test_zero_rescale_rows_and_zero_variance():
    eps = torch.randn(6, 5, 4, generator=torch.Generator().manual_seed(0))
    out = guidance_rescale(eps, [3.0, 5.0, 7.0], [0.5, 0.0, 1.0])
    assert torch.equal(out[1], eps[1].double()) and torch.equal(out[4], eps[4].double())
    assert torch.equal(out[0], out[3]) and torch.equal(out[2], out[5]) and not torch.equal(out[0], eps[0].double())
    flat = torch.full((2, 5, 4), 3.0)          # S_e == 0: the factor is 1 (diffusers: 0 / 0 -> NaN)
    assert torch.equal(guidance_rescale(flat, 7.5, 0.7), flat.double())


@pytest.mark.parametrize("phi", [0.0, 0.3, 0.7, 1.0])
def test_oracle_equals_the_literal_restatement(phi):
    """torch.std divides by N - 1, the oracle by nothing: the ratio does not see it"""
    gen = torch.Generator().manual_seed(3)
    B, H, W, g = 3, 6, 5, 7.5
    t = torch.randn(B, 4, H, W, generator=gen).double() + 0.4
    u = torch.randn(B, 4, H, W, generator=gen).double() * 0.8 - 0.2
    lit = rescale_noise_cfg_literal(u + g * (t - u), t, phi)
    eps = torch.cat([t, u]).permute(0, 2, 3, 1).reshape(2 * B, H * W, 4)
    if phi == 0.0:
        e, f = factors(eps, g, phi)
        mine = f.view(B, 1, 1) * e
        assert torch.equal(f, torch.ones(B).double())
    else:
        mine = guidance_rescale(eps, g, phi)[:B]
    want = lit.permute(0, 2, 3, 1).reshape(B, H * W, 4)
    assert (mine - want).abs().max() <= 1e-12 * want.abs().max()
