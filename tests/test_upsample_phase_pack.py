"""ops.pack_upsample_phase: nearest-2x upsample + 3x3 conv == four 2x2 phase convolutions on the SOURCE map with pre-summed weights
(csrc/conv_ups_phase.hip::conv_ups_phase_kernel).  For output phase (py, px)

    out[2y + py, 2x + px] = bias + sum_{dy, dx in {0, 1}} W'[py, px][dy, dx] . src[y + py - 1 + dy, x + px - 1 + dx]        (out-of-image src = 0)

The algebra is exact: checked in fp64 to 1e-12.  With W' rounded to 16 bits the result is no longer the direct form's bit for bit; its rms
error against fp64 (16-bit operands, fp32 accumulation, 16-bit output) must stay within 1.5 x the direct form's (measured 1.20 x / 1.25 x)."""
import pytest
import torch
import torch.nn.functional as F

from imagdressing_amd import ops


def pack_conv(w, cin_p):      # [Cout, Cin, 3, 3] -> [Cout, 9 * cin_p] (tap-major, channels zero-padded: unet.ConvOp's layout)
    w = w.permute(0, 2, 3, 1)
    return F.pad(w, (0, cin_p - w.shape[-1])).reshape(w.shape[0], -1).contiguous()


def phase_conv(x, wp, b):
    """x [B, Cp, H, W], wp [4, Cout, 4, Cp] (pack_upsample_phase's layout), b [Cout] -> [B, Cout, 2H, 2W], in x's dtype."""
    B, Cp, H, W = x.shape
    N = wp.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(B, N, 2 * H, 2 * W)
    for py in range(2):
        for px in range(2):
            k = wp[2 * py + px].view(N, 2, 2, Cp).permute(0, 3, 1, 2)            # [Cout, Cp, dy, dx]
            o = F.conv2d(xp, k, b)                                               # o[i, j] = sum W'[dy, dx] xp[i + dy, j + dx]: (H + 1) x (W + 1)
            out[:, :, py::2, px::2] = o[:, :, py:py + H, px:px + W]              # xp index = src index + 1 -> i = y + py, j = x + px
    return out


def direct(x, w, b):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 5, 7, 4, 12), (1, 8, 16, 32, 8), (1, 1, 1, 8, 4)])
def test_phase_form_is_exact_in_fp64(B, H, W, Cin, Cout):
    cin_p = (Cin + 7) // 8 * 8                                                   # Cin = 4 -> 8 packed channels
    x, w, b = rnd(1, B, Cin, H, W), rnd(2, Cout, Cin, 3, 3), rnd(3, Cout)
    wp = ops._pack_upsample_phase(pack_conv(w, cin_p))
    assert wp.dtype == torch.float64 and tuple(wp.shape) == (4, Cout, 4, cin_p)
    xq = F.pad(x, (0, 0, 0, 0, 0, cin_p - Cin), value=3.0)                       # whatever sits in the pad channels meets zero weights
    got, ref = phase_conv(xq, wp, b), direct(x, w, b)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("corner", [(0, 0), (0, 6), (4, 0), (4, 6)])
def test_one_hot_corners_pin_halo_and_phase_offsets(corner):
    H, W, Cin, Cout = 5, 7, 8, 4
    x = torch.zeros(1, Cin, H, W, dtype=torch.float64)
    x[0, 3, corner[0], corner[1]] = 1.0
    w = rnd(5, Cout, Cin, 3, 3)
    got, ref = phase_conv(x, ops._pack_upsample_phase(pack_conv(w, Cin)), None), direct(x, w, None)
    assert (ref != 0).sum().item() == Cout * 9                                   # a corner source pixel reaches a 3 x 3 block of output pixels
    assert (got - ref).abs().max().item() <= 1e-12
    assert torch.equal(got != 0, ref != 0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rounded_phase_weights_stay_within_the_direct_forms_error(dt):
    Cin, Cout, H, W = 320, 64, 12, 10
    x = rnd(11, 1, Cin, H, W).to(dt)
    w = (rnd(12, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5).to(dt)
    ref = direct(x.double(), w.double(), None)
    sigma = ref.std().item()
    d = direct(x.float(), w.float(), None).to(dt)
    wp = ops._pack_upsample_phase(pack_conv(w, Cin))                             # fp32 sums, rounded once to dt
    assert wp.dtype == dt
    p = phase_conv(x.float(), wp.float(), None).to(dt)
    rms = lambda t: ((t.double() - ref) ** 2).mean().sqrt().item() / sigma       # noqa: E731
    rd, rp = rms(d), rms(p)
    print(f"{dt}: direct rms {rd:.3e}, phase rms {rp:.3e}, ratio {rp / rd:.3f}")
    assert rp <= 1.5 * rd, (rd, rp)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_pack_from_fp32_weights_rounds_once(dt):
    """Packed from an fp32 weight (``dtype`` = the activation type) the summed taps carry one rounding, where packing the 16-bit weight rounds twice.
    Against the exact sums the single rounding is the rounding of the result type alone (half an ulp), and smaller in rms than the double one."""
    w = (rnd(21, 16, 9 * 32) * 0.05).float()
    exact = ops._pack_upsample_phase(w.double())
    once = ops._pack_upsample_phase(w, dt)
    twice = ops._pack_upsample_phase(w.to(dt))
    assert once.dtype == twice.dtype == dt and once.shape == exact.shape
    ulp = torch.finfo(dt).eps * exact.abs().clamp(min=float(torch.finfo(dt).tiny))
    assert bool(((once.double() - exact).abs() <= 0.5 * ulp * (1 + 1e-6) + 1e-9 * exact.abs()).all())     # (fp32 sums of four terms: 1e-7 relative)
    rms = lambda t: ((t.double() - exact) ** 2).mean().sqrt().item()               # noqa: E731
    assert rms(once) < 0.85 * rms(twice), (rms(once), rms(twice))


def test_pack_is_cached_per_weight_and_version():
    w = rnd(7, 8, 9 * 8).to(torch.bfloat16)
    p = ops.pack_upsample_phase(w)
    assert ops.pack_upsample_phase(w) is p and tuple(p.shape) == (4, 8, 4, 8) and p.dtype == w.dtype
    w.mul_(2.0)                                                                  # new version of the same storage -> packed again
    q = ops.pack_upsample_phase(w)
    assert q is not p and torch.equal(q.float(), 2.0 * p.float())
    with pytest.raises(ops.L.ImdError):
        ops.pack_upsample_phase(torch.zeros(8, 10))


def test_query_without_gpu():
    """imd_conv_ups_phase_supported is a pure predicate over the parameter block."""
    import ctypes
    lib = ops.L.load()
    ask = lambda p: lib.imd_conv_ups_phase_supported(ctypes.byref(p))            # noqa: E731
    blk = lambda shape, N: ops._ups_phase_block(shape, N, torch.bfloat16)        # noqa: E731
    assert ask(blk((4, 32, 32, 640), 640)) == 1 and ask(blk((8, 16, 16, 1280), 1280)) == 1 and ask(blk((4, 256, 256, 256), 256)) == 1
    assert ask(blk((8, 8, 8, 1280), 1280)) == 0                                  # 16 multiply units against the 18 of the 16 x 16 output map (320 workgroups)
    # a grid below 160 workgroups does not pay against the K-sliced 9-tap launch (the launcher would still run these)
    assert ask(blk((1, 32, 32, 640), 640)) == 1 and ask(blk((2, 16, 16, 1280), 1280)) == 1          # 160 each: measured gains
    assert ask(blk((1, 16, 16, 1280), 1280)) == 0                                # 80: measured none
    assert ask(blk((1, 12, 9, 64), 128)) == 0 and ask(blk((2, 9, 18, 96), 160)) == 0 and ask(blk((4, 8, 12, 160), 160)) == 0
    assert ask(blk((2, 16, 16, 24), 64)) == 0                                    # Cin % 32
    for field, bad in (("res", 0x10000), ("rowvec", 0x10000), ("gn_a", 0x10000), ("gn_stats_out", 0x10000), ("act", 1), ("split_k", 2), ("out_f32", 1),
                       ("stride", 2), ("ups", 0), ("Hout", 63), ("x_pix_stride", 648), ("out_ld", 1280), ("out_scale", 0.5), ("mode", 1)):
        p = blk((4, 32, 32, 640), 640)
        setattr(p, field, bad)
        assert ask(p) == 0, field
    p = blk((4, 32, 32, 640), 640)
    p.struct_bytes -= 8
    assert ask(p) == 0 and lib.imd_conv_ups_phase(ctypes.byref(p), None) != 0 and b"parameter block is" in lib.imd_last_error()
