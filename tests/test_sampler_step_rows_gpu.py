"""The per-row fused sampler step on the GPU (``imd_sampler_step_rows``): every latent row with its own coefficient block, history
slot and active flag, against ``imd_sampler_step`` run on that row alone -- bit for bit, the per-pixel arithmetic is the same -- and
an inactive row keeps every byte of its latent, history and next-input pixels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def g(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _row_coefs(b, K):
    """a different block for every row b; the store slot differs too: K = 4 -> slots 0, 1, 2; K = 1 -> 0, none, 0; K = 0 -> none"""
    from imagdressing_amd import ops
    zh = [0.7, -0.3, 0.45, -0.2][:K]
    return ops.sampler_coefs(m_x=1.2 + 0.1 * b, m_e=-0.8 - 0.05 * b, z_x=0.9 - 0.07 * b, z_m=0.35 + 0.03 * b, z_h=[c * (1 + 0.2 * b) for c in zh],
                             z_n=0.6 + 0.1 * b, b_img=0.95 - 0.02 * b, b_noise=0.3 + 0.04 * b, in_scale=0.37 + 0.11 * b,
                             store=(b + 1) % (K + 1) - 1)


CASES = [(B, HW, K) for (B, HW) in [(1, 1), (3, 77), (2, 300)] for K in (0, 1, 4)] + [(2, 270000, 1)]
IDS = [f"{name}-K{K}" for name in ("lone", "partial-block", "row-boundary") for K in (0, 1, 4)] + ["second-pass-K1"]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,HW,K", CASES, ids=IDS)
def test_sampler_step_rows_kernel(B, HW, K, dtype):
    """a lone element, a partial block, a row boundary inside a block, and 2 x 270000 pixels (more than the 2048 x 256 a grid covers
    in one pass: the threads that wrap around land in the other row, so the row's block must be read per pixel, not per thread)."""
    from imagdressing_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = "cuda"
    z0, eps = g(1, B, HW, 4).to(dev), g(2, 2 * B, HW, 4).to(dev)
    H0 = g(3, K, B, HW, 4).to(dev)                          # (random values: the sentinel of the history slots)
    noise, z_img, bn = g(4, B, HW, 4).to(dev), g(5, B, HW, 4).to(dev), g(6, B, HW, 4).to(dev)
    mask = (torch.rand(B, HW, generator=torch.Generator().manual_seed(7)) > 0.4).float()
    mask[0, 0] = 0.25                                       # a fractional value too
    mask = mask.to(dev)
    g_mixed = torch.tensor([5.0, 7.5, 9.0][:B])
    coefs = [_row_coefs(b, K) for b in range(B)]
    if K == 4 and B == 3:
        assert len({c[12] for c in coefs}) == 3 and all(coefs[a][:12] != coefs[b][:12] for a in range(B) for b in range(a))

    def launch(rows, guidance, use_noise, use_blend, fn=None, **over):
        z, H = z0.clone(), (H0.clone() if K else None)
        xn = torch.full((2 * B, HW, 8), SENTINEL, dtype=dtype, device=dev)
        kw = dict(mask=mask, z_img=z_img, blend_noise=bn) if use_blend else {}
        if fn is None:
            ops.sampler_step_rows(z, eps, xn, guidance=guidance, coef_rows=torch.tensor(rows, dtype=torch.float32, device=dev), hist=H,
                                  noise=noise if use_noise else None, **kw)
        else:
            fn(z, eps, xn, guidance=guidance, hist=H, noise=noise if use_noise else None, **kw, **over)
        return z, H, xn

    def solo(b, use_noise, use_blend):
        """imd_sampler_step on row b alone: its CFG pair of eps rows, its column of every history slot, the host coefficients"""
        z, H = z0[b:b + 1].clone(), (H0[:, b:b + 1].clone() if K else None)
        xn = torch.full((2, HW, 8), SENTINEL, dtype=dtype, device=dev)
        kw = dict(mask=mask[b:b + 1].contiguous(), z_img=z_img[b:b + 1].contiguous(), blend_noise=bn[b:b + 1].contiguous()) if use_blend else {}
        ops.sampler_step(z, torch.cat([eps[b:b + 1], eps[B + b:B + b + 1]]), xn, guidance=float(g_mixed[b]), coefs=coefs[b], hist=H,
                         noise=noise[b:b + 1].contiguous() if use_noise else None, **kw)
        return z, H, xn

    for use_noise in (False, True):
        for use_blend in (False, True):
            what = (B, HW, K, use_noise, use_blend)
            z, H, xn = launch([ops.sampler_coef_row(c) for c in coefs], g_mixed.to(dev), use_noise, use_blend)
            assert torch.isfinite(z).all(), what
            solos = [solo(b, use_noise, use_blend) for b in range(B)]
            for b, (zb, Hb, xb) in enumerate(solos):
                assert torch.equal(z[b], zb[0]), (what, b)
                assert torch.equal(xn[b], xb[0]) and torch.equal(xn[B + b], xb[1]), (what, b)
                assert K == 0 or torch.equal(H[:, b], Hb[:, 0]), (what, b)
                assert not torch.equal(zb[0], z0[b])                               # (the step really moved the row)
            # each row in turn inactive: all of its bytes stay, the other rows are what they were
            for r in range(B):
                rows = [ops.sampler_coef_row(c, active=(b != r)) for b, c in enumerate(coefs)]
                zi, Hi, xi = launch(rows, g_mixed.to(dev), use_noise, use_blend)
                assert torch.equal(zi[r], z0[r]) and (K == 0 or torch.equal(Hi[:, r], H0[:, r])), (what, r)
                assert (xi[r] == SENTINEL).all() and (xi[B + r] == SENTINEL).all(), (what, r)
                for b in range(B):
                    if b != r:
                        assert torch.equal(zi[b], z[b]) and torch.equal(xi[b], xn[b]) and torch.equal(xi[B + b], xn[B + b]), (what, r, b)
                        assert K == 0 or torch.equal(Hi[:, b], H[:, b]), (what, r, b)
            # all rows equal and active == imd_sampler_step, host-coefficient and device-coefficient form
            c = _row_coefs(1, K)
            zr, Hr, xr = launch([ops.sampler_coef_row(c)] * B, 7.5, use_noise, use_blend)
            for form in (c, torch.tensor(c, dtype=torch.float32, device=dev)):
                zs, Hs, xs = launch(None, 7.5, use_noise, use_blend, fn=ops.sampler_step, coefs=form)
                assert torch.equal(zr, zs) and torch.equal(xr, xs) and (K == 0 or torch.equal(Hr, Hs)), what
            zu, Hu, xu = launch([ops.sampler_coef_row(c)] * B, torch.full((B,), 7.5, device=dev), use_noise, use_blend)
            assert torch.equal(zr, zu) and torch.equal(xr, xu) and (K == 0 or torch.equal(Hr, Hu)), what


def test_sampler_step_rows_refusals_keep_the_latent():
    """errors, and nothing launched: the latent keeps its bits"""
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    B, HW = 2, 40
    z0, eps = g(1, B, HW, 4).cuda(), g(2, 2 * B, HW, 4).cuda()
    xn = torch.zeros(2 * B, HW, 8, dtype=torch.float16, device="cuda")
    rows = torch.tensor([ops.sampler_coef_row(ops.sampler_coefs(z_x=0.5))] * B, dtype=torch.float32, device="cuda")
    z = z0.clone()
    for bad in (rows[:1], rows.double(), rows.cpu().tolist(), torch.zeros(B + 1, 16, device="cuda")[1:, :16].t().contiguous().t()):
        with pytest.raises(ImdError, match="coef_rows"):
            ops.sampler_step_rows(z, eps, xn, guidance=7.5, coef_rows=bad)
    with pytest.raises(ImdError, match="16-byte"):
        ops.sampler_step_rows(z, eps, xn, guidance=7.5, coef_rows=torch.zeros(B * 16 + 1, device="cuda")[1:].view(B, 16))
    with pytest.raises(ImdError, match="hist"):
        ops.sampler_step_rows(z, eps, xn, guidance=7.5, coef_rows=rows, hist=torch.zeros(5, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(z, z0)
    ops.sampler_step_rows(z, eps, xn, guidance=7.5, coef_rows=rows)
    assert not torch.equal(z, z0)
