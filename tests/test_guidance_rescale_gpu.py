"""imd_guidance_rescale on the GPU (csrc/guidance_rescale.hip):

* the EXACT families of tests/guidance_rescale_cases.py (preconditions asserted on the CPU in test_guidance_rescale_inputs.py):
  ``torch.equal`` on both CFG halves, scalar and per-row g and phi, whatever the reduction order;
* rows with phi = 0 keep their bytes (a NaN-filled pair included), sentinel rows around eps stay untouched;
* a row's output does not depend on B, on its position or on which other rows are active;
* Gaussian inputs with a mean offset against the float64 oracle fed the same fp32 inputs, within a DERIVED bound;
* composition: after the launch each of the three step kernels recovers e' whatever guidance it is given.

Shapes are the kernel's edge cases (cases.HW_SIZES): around a wave and a quarter workgroup, not a multiple of the 1024-pixel thread
stride, and either side of the register-resident / re-read boundary (8192 pixels)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import guidance_rescale_cases as cases  # noqa: E402
from tests.guidance_rescale_oracle import factors, guidance_rescale as oracle  # noqa: E402

SENTINEL = 12345.0


def chain(HW):
    """L: the longest chain of sequential fp32 additions in the kernel's reduction (guidance_rescale.hip): a thread's pixels (1024
    threads, stride 1024), the three additions inside one pixel's squared deviations, six butterfly steps over the wave, fifteen
    additions over the sixteen wave partials"""
    return math.ceil(HW / 1024) + 3 + 6 + 15


def run(eps, g, phi):
    """one launch on a device copy framed by sentinel rows -> the rescaled eps (on the host); the sentinels are checked"""
    from imagdressing_amd import ops
    rows, HW = eps.shape[0], eps.shape[1]
    buf = torch.full((rows + 2, HW, 4), SENTINEL, dtype=torch.float32).cuda()
    buf[1:rows + 1].copy_(eps)
    view = buf[1:rows + 1]
    dev = lambda v: torch.tensor(v, dtype=torch.float32).cuda() if isinstance(v, (list, tuple)) else v
    assert ops.guidance_rescale(view, guidance=dev(g), rescale=dev(phi)) is view
    torch.cuda.synchronize()
    out = buf.cpu()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all()
    return out[1:rows + 1]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("HW", cases.HW_SIZES)
def test_exact_families(HW):
    for g in cases.GS:
        for phi in cases.PHIS:
            eps, want = cases.build("A", HW, g, phi)
            assert torch.equal(run(eps, g, phi), want), ("A", HW, g, phi)
    for phi in cases.PHIS + (0.7,):
        if phi != 0.7:
            eps, want = cases.build("B", HW, 8.0, phi)
            assert torch.equal(run(eps, 8.0, phi), want), ("B", HW, phi)
        for g in (2.0, 7.5):
            eps, want = cases.build("C", HW, g, phi)
            assert torch.equal(run(eps, g, phi), want), ("C", HW, g, phi)
    # per row: B = 3, g and phi from device arrays -- both, and each beside a scalar
    g3, p3 = [2.0, 4.0, 8.0], [1.0, 0.5, 0.25]
    for fam in ("A", "B"):
        eps, want = cases.build(fam, HW, g3, p3, B=3)
        assert torch.equal(run(eps, g3, p3), want), (fam, HW, "rows")
        eps, want = cases.build(fam, HW, 4.0, p3, B=3)
        assert torch.equal(run(eps, 4.0, p3), want), (fam, HW, "phi rows")
        eps, want = cases.build(fam, HW, g3, 0.5, B=3)
        assert torch.equal(run(eps, g3, 0.5), want), (fam, HW, "g rows")


@pytest.mark.parametrize("HW", [1, 65, 257, 8193])
def test_rows_with_zero_rescale_keep_their_bytes(HW):
    """phi = [a, 0, b]: the middle pair is byte-identical to its input -- Gaussian, and NaN-filled (an idle session slot may hold
    anything; NaN payloads survive only if the row is not rewritten)"""
    gen = torch.Generator().manual_seed(HW)
    eps = torch.randn(6, HW, 4, generator=gen) + 0.3
    for fill in (None, float("nan")):
        if fill is not None:
            eps[1] = fill
            eps[4] = torch.tensor([0x7fc12345], dtype=torch.int32).view(torch.float32)          # a NaN with a payload
        out = run(eps, [3.0, 5.0, 7.5], [0.7, 0.0, 0.25])
        assert torch.equal(bits(out[1]), bits(eps[1])) and torch.equal(bits(out[4]), bits(eps[4]))
        for b in (0, 2):
            assert torch.isfinite(out[b]).all() and torch.equal(out[b], out[3 + b]) and not torch.equal(out[b], eps[b])
    # all rows 0 through the device array: nothing changes at all
    assert torch.equal(bits(run(eps, 7.5, [0.0, 0.0, 0.0])), bits(eps))


@pytest.mark.parametrize("HW", [3, 64, 257, 1025, 8192, 8193])
def test_a_row_does_not_depend_on_its_batch(HW):
    gen = torch.Generator().manual_seed(100 + HW)
    t, u = torch.randn(1, HW, 4, generator=gen) * 1.3 + 0.4, torch.randn(1, HW, 4, generator=gen) - 0.2
    ot, ou = torch.randn(2, HW, 4, generator=gen), torch.randn(2, HW, 4, generator=gen)
    alone = run(torch.cat([t, u]), 7.5, 0.7)
    assert torch.equal(alone[0], alone[1]) and not torch.equal(alone[0], t[0])
    for pos in range(3):
        order = [0, 1]
        order.insert(pos, None)
        cond = torch.cat([t if k is None else ot[k:k + 1] for k in order])
        unc = torch.cat([u if k is None else ou[k:k + 1] for k in order])
        for others in (0.5, 0.0):
            g = [7.5 if k is None else 3.0 for k in order]
            phi = [0.7 if k is None else others for k in order]
            out = run(torch.cat([cond, unc]), g, phi)
            assert torch.equal(out[pos], alone[0]) and torch.equal(out[3 + pos], alone[0]), (HW, pos, others)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", cases.HW_SIZES)
def test_gaussian_rows_against_the_float64_oracle(HW, B):
    """The bar is derived.  S_t and S_e are sums of non-negative terms, each term carrying a few roundings and the sum at most L
    sequential additions: relative error <= (L + 4) u each, u = 2^-24 (the rounded means move a centred sum at second order only).
    Their ratio, the correctly rounded division and square root and the fused phi r + (1 - phi) add less than 4 u, the ratio's two
    errors halve under the root: f is within (L + 8) u = (L / 2 + 4) 2^-23 of the oracle's, inside the (L + 16) 2^-23 asserted.
    Elements: e = fma(g, t - u, u) is two roundings of quantities bounded by |u| + g |t - u|, then one for f e."""
    gen = torch.Generator().manual_seed(1000 * B + HW)
    t = torch.randn(B, HW, 4, generator=gen) * 1.2 + 0.5
    u = torch.randn(B, HW, 4, generator=gen) * 0.9 + 0.35
    eps = torch.cat([t, u])
    gs, ps = [7.5, 3.0, 12.0][:B], [0.7, 1.0, 0.3][:B]
    out = run(eps, gs if B > 1 else gs[0], ps if B > 1 else ps[0]).double()
    want = oracle(eps, gs, ps)
    e, f = factors(eps, gs, ps)
    fbar = (chain(HW) + 16) * 2.0 ** -23
    g = torch.tensor(gs).double().view(B, 1, 1)
    bound = fbar * want[:B].abs() + 2.0 ** -22 * (u.double().abs() + g * (t.double() - u.double()).abs()) * f.view(B, 1, 1)
    err = (out[:B] - want[:B]).abs()
    print(f"guidance_rescale HW={HW} B={B}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert torch.equal(out[:B], out[B:]) and (err <= bound).all()
    # the factor itself, where e is exact (u = 0, g = 2): out / e is f up to the one rounding of the product
    eps0 = torch.cat([t, torch.zeros_like(t)])
    out0 = run(eps0, 2.0, ps if B > 1 else ps[0]).double()
    e0, f0 = factors(eps0, 2.0, ps)
    rel = ((out0[:B] / e0 - f0.view(B, 1, 1)) / f0.view(B, 1, 1)).abs().max().item()
    print(f"  factor: max relative error {rel / 2.0 ** -23:.3f} x 2^-23, bar {chain(HW) + 16} (+ 1/2 for the product)")
    assert rel <= fbar + 2.0 ** -24


@pytest.mark.parametrize("HW", [65, 1025])
def test_every_step_kernel_recovers_the_rescaled_prediction(HW):
    """guidance_rescale, then a step at guidance g  ==  the same step at guidance 1.0 on the eps the launch left (e' in both halves):
    eps_u + g (eps_c - eps_u) with eps_c == eps_u is eps_u for every g"""
    from imagdressing_amd import ops
    B, g = 2, 7.5
    gen = torch.Generator().manual_seed(HW)
    z0 = torch.randn(B, HW, 4, generator=gen)
    eps = torch.cat([torch.randn(B, HW, 4, generator=gen) + 0.5, torch.randn(B, HW, 4, generator=gen)]).cuda()
    ops.guidance_rescale(eps, guidance=g, rescale=0.7)
    assert torch.equal(eps[:B], eps[B:])
    hist0 = torch.randn(3, B, HW, 4, generator=gen)
    steps = {
        "ddim": lambda z, x, gd: ops.ddim_cfg_step(z, eps, x, guidance=gd, a_t=0.5, a_prev=0.7),
        "sampler": lambda z, x, gd: ops.sampler_step(z, eps, x, guidance=gd, hist=hist0.clone().cuda(),
                                                     coefs=ops.sampler_coefs(0.8, -0.6, 0.5, 0.4, (0.3, -0.2), in_scale=0.9, store=2)),
        "unipc": lambda z, x, gd: ops.unipc_step(z, eps, x, guidance=gd, hist=hist0.clone().cuda(),
                                                 coefs=ops.unipc_coefs(0.8, -0.6, 0.2, 0.5, (0.3, 0.1), 0.7, 0.4, (0.2, -0.1), in_scale=0.9,
                                                                       store_m=2, store_s=1)),
    }
    for name, step in steps.items():
        outs = []
        for gd in (g, 1.0):
            z, x = z0.clone().cuda(), torch.zeros(2 * B, HW, 8, dtype=torch.float16).cuda()
            step(z, x, gd)
            torch.cuda.synchronize()
            outs.append((z.cpu(), x.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), name
        assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], z0), name
