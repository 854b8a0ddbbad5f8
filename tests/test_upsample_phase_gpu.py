"""Nearest-2x upsample + 3x3 conv as four 2x2 phase convolutions (csrc/conv_ups_phase.hip::conv_ups_phase_kernel, ops.conv_ups_phase) against
F.conv2d(F.interpolate(x, 2, 'nearest'), w, b, padding=1) and against the 9-tap path it replaces (ops.conv2d_nhwc(ups=True), what
IMD_UPS_PHASE=0 runs).

Bars.  Integer data: every product and sum is exact in fp32 and the pre-summed weights (|W'| <= 8) are exact in 16 bits, so the output must
equal the fp32 reference rounded to 16 bits, and the 9-tap path's output, bit for bit.  Random data: the rms error against fp64 on the same
16-bit operands must stay within 1.5 x the 9-tap path's (rounding W' once more adds an error of about the size of the output rounding, i.e.
a ratio of about sqrt(2); tests/test_upsample_phase_pack.py measures 1.42 on the CPU), and every element must sit inside the TOL of the
existing conv tests (tests/test_kernels_gpu.py).  The 1.5 x bar is on the rms, as in the CPU test: a maximum over 10^5 outputs of two different
error distributions has a sampling spread of its own, and the per-element TOL bounds it.

Measured (MI355X, four shapes): rms phase / 9-tap bf16 2.78e-3 .. 2.81e-3 / 2.25e-3 .. 2.30e-3 (1.22 .. 1.23 x), fp16 3.46e-4 .. 3.52e-4 / 2.82e-4 .. 2.87e-4
(1.22 .. 1.23 x); max bf16 1.70e-2 .. 2.01e-2 / 1.56e-2, fp16 2.21e-3 .. 2.63e-3 / 1.95e-3.  Small models, switch on against off: UNet rel-rms 8.6e-3 bf16 /
1.07e-3 fp16, VAE decode 9.6e-3 / 1.20e-3.  The small models above ran a 32 x 32-latent UNet and an 8 x 8-latent VAE before the query had
its grid clause.  With every layer the kernel can run on the phase path, all whole-model bars of the suite held except the max-abs of two bf16 inpainting
trajectories of the small model (tests/test_e2e_gpu.py::test_pipeline_inpaint_small[bf16] 1.121 against 0.902, 0.748 with the switch off, rel-rms 0.0182 / 0.0188;
tests/test_multi_request_gpu.py::test_inpainting_two_requests_strength[bf16] 0.318 against 0.272): 32-workgroup layers that gain no time, which the query now leaves
on the 9-tap launch (fewer than 160 workgroups: DESIGN.md sections 2.2g and 6).  The kernel cases below call the launch directly; it runs any grid."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
TOL = {torch.bfloat16: 1e-2, torch.float16: 2e-3}          # tests/test_kernels_gpu.py
# B, source H x W, Cin, Cout
CASES = [(2, 8, 16, 32, 128),       # one tile, one chunk
         (2, 9, 18, 96, 160),       # tiles overhang both ways; three chunks (odd: the loop leaves mid-period); ragged channel tile with a dead wave
         (1, 12, 9, 64, 128),       # the 768 x 576 geometry's W < 16
         (3, 16, 32, 320, 320)]     # several pixel and channel tiles, 10 chunks (past one period of the unrolled loop)
CASE = pytest.mark.parametrize("B,H,W,Cin,Cout", CASES, ids=[f"{b}x{h}x{w}x{ci}-{co}" for b, h, w, ci, co in CASES])
SENTINEL = -123.0
_REF = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def pack_conv(w):  # [Cout, Cin, 3, 3] -> [Cout, 9 * Cin]
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def reference(x, w, b, dtype):
    """conv3x3(nearest2x(x)) + b in ``dtype`` on the CPU, NHWC."""
    xin = F.interpolate(x.to(dtype), scale_factor=2, mode="nearest")
    return F.conv2d(xin, w.to(dtype), b.to(dtype), padding=1).permute(0, 2, 3, 1).contiguous()


def case_data(kind, B, H, W, Cin, Cout, dt):
    """Inputs and CPU references of a case, computed once per session and left unchanged."""
    key = (kind, B, H, W, Cin, Cout, dt)
    if key not in _REF:
        if kind == "int":
            x = torch.randint(-4, 5, (B, Cin, H, W), generator=gen(1)).to(dt)
            w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=gen(2)).to(dt)
            b = torch.randint(-3, 4, (Cout,), generator=gen(3)).float()
            ref = reference(x, w, b, torch.float32)
        else:
            x = torch.randn(B, Cin, H, W, generator=gen(4)).to(dt)
            w = (torch.randn(Cout, Cin, 3, 3, generator=gen(5)) * (9 * Cin) ** -0.5).to(dt)
            b = torch.randn(Cout, generator=gen(6))
            ref = reference(x, w, b, torch.float64)
        _REF[key] = (x.permute(0, 2, 3, 1).contiguous().cuda(), pack_conv(w).cuda(), b.cuda(), ref)
    return _REF[key]


def run_phase(ops, x, w, b):
    """The phase launch into a buffer with a sentinel tail -> (output, tail)."""
    B, H, W, _ = x.shape
    n = 4 * B * H * W * w.shape[0]
    buf = torch.full((n + 4096,), SENTINEL, dtype=x.dtype, device=x.device)
    out = ops.conv_ups_phase(x, w, b, out=buf[:n].view(B, 2 * H, 2 * W, w.shape[0]))
    return out, buf[n:]


@CASE
@DTS
def test_integer_data_is_bit_exact(ops, B, H, W, Cin, Cout, dt):
    x, w, b, ref = case_data("int", B, H, W, Cin, Cout, dt)
    out, tail = run_phase(ops, x, w, b)
    want = ref.to(dt)                       # the exact fp32 value, rounded once
    assert out.shape == want.shape and out.dtype == dt
    bad = (out.cpu() != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ from the exact result; first at (b, y, x, n) = {bad[0].tolist()}"
    assert torch.equal(out, ops.conv2d_nhwc(x, w, b, ups=True)), "differs from the 9-tap path on exact data"
    assert bool((tail == SENTINEL).all()), "wrote past the end of the output"
    again, tail = run_phase(ops, x, w, b)
    assert torch.equal(again, out) and bool((tail == SENTINEL).all())


@CASE
@DTS
def test_random_data_against_fp64_and_the_9_tap_path(ops, B, H, W, Cin, Cout, dt):
    x, w, b, ref = case_data("rnd", B, H, W, Cin, Cout, dt)
    out, tail = run_phase(ops, x, w, b)
    nine = ops.conv2d_nhwc(x, w, b, ups=True)
    err = lambda t: (t.double().cpu() - ref)            # noqa: E731
    rms = lambda t: err(t).pow(2).mean().sqrt().item()  # noqa: E731
    r_phase, r_nine = rms(out), rms(nine)
    print(f"{B}x{H}x{W}x{Cin}->{Cout} {dt}: rms phase {r_phase:.3e} / 9-tap {r_nine:.3e} = {r_phase / r_nine:.3f}; "
          f"max phase {err(out).abs().max().item():.3e} / 9-tap {err(nine).abs().max().item():.3e}")
    assert r_phase <= 1.5 * r_nine, (r_phase, r_nine)
    e = err(out).abs()
    assert bool((e <= TOL[dt] + TOL[dt] * ref.abs()).all()), f"max abs error {e.max().item():.4g} outside atol = rtol = {TOL[dt]}"
    assert bool((tail == SENTINEL).all()), "wrote past the end of the output"
    again, _ = run_phase(ops, x, w, b)
    assert torch.equal(again, out)


def test_query_refuses_what_the_kernel_does_not_take(ops):
    lib = ops.L.load()
    dt = torch.bfloat16
    x = lambda *s: torch.zeros(*s, dtype=dt, device="cuda")         # noqa: E731
    assert ops.conv_ups_phase_supported(x(8, 32, 32, 64), x(128, 9 * 64))            # 8 images x 8 tiles x 4 phases = 256 workgroups
    assert not ops.conv_ups_phase_supported(x(64, 8, 8, 64), x(128, 9 * 64))         # an 8 x 8 source: the half-empty tile eats the gain (256 workgroups)
    assert not ops.conv_ups_phase_supported(x(8, 32, 32, 24), x(128, 9 * 24))        # Cin % 32
    assert not ops.conv_ups_phase_supported(x(2, 16, 32, 64), x(128, 9 * 64))        # 32 workgroups: no gain over the K-sliced 9-tap launch
    p = ops._ups_phase_block((8, 32, 32, 64), 128, dt)
    assert lib.imd_conv_ups_phase_supported(ctypes.byref(p)) == 1
    p.res = 0x10000                                                                    # a residual (never dereferenced by the query)
    assert lib.imd_conv_ups_phase_supported(ctypes.byref(p)) == 0
    with pytest.raises(ops.L.ImdError):                                                # no quiet fall-back inside the launch wrapper
        ops.conv_ups_phase(x(2, 16, 32, 24), x(128, 9 * 24))


# per-forward bars of tests/test_e2e_gpu.py (small UNet) and tests/test_vae_gpu.py (small VAE)
UNET_BARS = {torch.float16: dict(max_abs=1e-2, rel_rms=4e-3), torch.bfloat16: dict(max_abs=5e-2, rel_rms=2e-2)}
VAE_BARS = {torch.float16: dict(rel_rms=5e-3, max_rel=2.5e-2), torch.bfloat16: dict(rel_rms=2.5e-2, max_rel=0.15)}


def _on_off(ops, monkeypatch, fn):
    """fn() with the switch on (the event hook must see phase launches) and off (it must see none) -> (on, off, phase launches)."""
    monkeypatch.setattr(ops, "UPS_PHASE", True)
    monkeypatch.setattr(ops, "GEMM_EVENT_HOOK", {})
    on = fn()
    n_on = sum(len(v) for k, v in ops.GEMM_EVENT_HOOK.items() if k[1] == ops.UPS_PHASE_CFG)
    monkeypatch.setattr(ops, "UPS_PHASE", False)
    monkeypatch.setattr(ops, "GEMM_EVENT_HOOK", {})
    off = fn()
    assert not any(k[1] == ops.UPS_PHASE_CFG for k in ops.GEMM_EVENT_HOOK)
    return on, off, n_on


@DTS
@torch.no_grad()
def test_small_unet_and_vae_switch_on_against_off(ops, monkeypatch, dt):
    from imagdressing_amd.vae import AutoencoderKL
    from tests.harness import SMALL, build_pair, err_stats
    p = build_pair(SMALL, seed=0, dtype=dt)
    # four 64 x 64 latents: the last upsampler (160 channels, 32 x 32 -> 64 x 64: 4 x 8 tiles x 4 phases x 2 channel tiles = 256 workgroups) is one the
    # query accepts; the two below it (8 x 8 source; 16 x 16 source with 96 workgroups) are not
    x = torch.randn(4, 4, 64, 64, generator=gen(1)).cuda()
    ehs = (torch.randn(4, 77, 64, generator=gen(2)) * 0.5).cuda()
    on, off, n = _on_off(ops, monkeypatch, lambda: p["e_unet"](x, 481, ehs)[0])
    assert n == 1, f"expected one phase launch in the small UNet, the hook saw {n}"
    st = err_stats(on, off)
    print(f"small UNet {dt}: on vs off {st}")
    assert st["max_abs"] < UNET_BARS[dt]["max_abs"] and st["rel_rms"] < UNET_BARS[dt]["rel_rms"], st
    vcfg = dict(block_out_channels=(64, 128, 128, 128), norm_num_groups=8)
    vae = AutoencoderKL.random_init(seed=5, config=vcfg, device="cuda", dtype=dt)
    z = torch.randn(2, 4, 16, 16, generator=gen(3)).cuda()
    on, off, n = _on_off(ops, monkeypatch, lambda: vae.decode(z, return_dict=False)[0])
    assert n == 1, f"expected one phase launch in the small VAE decode (the 64 x 64 source: 256 workgroups; 16 and 64 below it), the hook saw {n}"
    st = err_stats(on, off)
    print(f"small VAE decode {dt}: on vs off {st}")
    assert st["rel_rms"] < VAE_BARS[dt]["rel_rms"] and st["max_abs"] < VAE_BARS[dt]["max_rel"] * st["ref_std"], st
