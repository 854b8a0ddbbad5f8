"""FreeU (Si et al., CVPR 2024) restated from diffusers 0.24 ``utils/torch_utils.py`` (``fourier_filter`` / ``apply_freeu``) in float64,
the closed form the HIP kernel computes, the integer-valued cases whose answer is known exactly, and the mutations the exact comparison
must catch.  CPU only: torch on the host, nothing of the package is imported at module level.  diffusers is not installed here, so the
restatement itself is unpinned (as the UniPC oracle's is).

``fourier_filter(x, threshold=1, scale=s)``: fftn over (H, W), fftshift, the 2 x 2 block [H//2-1 : H//2+1, W//2-1 : W//2+1] times s,
ifftshift, ifftn, real part.  The block holds ky in {0, -1 mod H}, kx in {0, -1 mod W} as SETS, hence the closed form

    y = x + (s - 1) / (H W) * sum over the waves of  A cos(phi) + B sin(phi),   A = sum x cos(phi),  B = sum x sin(phi)

with the waves: the mean; the row wave phi = 2 pi n / H when H > 1; the column wave 2 pi m / W when W > 1; the diagonal 2 pi (n / H + m / W)
when both (A cos + B sin is even in phi, so -1 and +1 give the same term)."""
import math
import types

import torch

F64 = torch.float64
MAP_SIZES = [(1, 1), (1, 2), (2, 2), (2, 4), (3, 5), (4, 4), (4, 8), (6, 10), (8, 8), (8, 10), (16, 20), (32, 40), (5, 1)]


# ---- the filter -----------------------------------------------------------------------------------------------------------------------------------
def fourier_filter_ref(x: torch.Tensor, threshold: int, scale: float) -> torch.Tensor:
    """x [..., H, W] -> float64, the literal FFT form."""
    x = x.to(F64)
    H, W = x.shape[-2:]
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(H, W, dtype=F64)
    crow, ccol = H // 2, W // 2
    mask[crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    xf = xf * mask
    return torch.fft.ifftn(torch.fft.ifftshift(xf, dim=(-2, -1)), dim=(-2, -1)).real


def closed_form(x: torch.Tensor, scale: float, anti: bool = False, double: bool = False) -> torch.Tensor:
    """x [..., H, W] -> float64, the seven-sum form.  Mutations: ``anti`` uses the anti-diagonal wave cos(a - b) in place of cos(a + b);
    ``double`` keeps the row / column / diagonal waves on one-row and one-column maps (a frequency counted twice)."""
    x = x.to(F64)
    H, W = x.shape[-2:]
    n = torch.arange(H, dtype=F64)[:, None] / H
    m = torch.arange(W, dtype=F64)[None, :] / W
    zero = torch.zeros(H, W, dtype=F64)
    waves = [zero]
    if H > 1 or double:
        waves.append(2 * math.pi * n + zero)
    if W > 1 or double:
        waves.append(2 * math.pi * m + zero)
    if (H > 1 and W > 1) or double:
        waves.append(2 * math.pi * ((n - m) if anti else (n + m)))
    y = x.clone()
    for phi in waves:
        c, s = torch.cos(phi), torch.sin(phi)
        A = (x * c).sum((-2, -1), keepdim=True)
        B = (x * s).sum((-2, -1), keepdim=True)
        y = y + (scale - 1.0) / (H * W) * (A * c + B * s)
    return y


def apply_freeu_ref(block: int, hidden: torch.Tensor, skip: torch.Tensor, s1: float, s2: float, b1: float, b2: float):
    """NCHW ``apply_freeu`` of up block ``block``: blocks 0 and 1 scale the lower channel half of the backbone and filter the skip."""
    if block not in (0, 1):
        return hidden, skip
    b, s = (b1, s1) if block == 0 else (b2, s2)
    half = hidden.shape[1] // 2
    hidden = torch.cat([hidden[:, :half] * b, hidden[:, half:]], 1)
    return hidden, fourier_filter_ref(skip, 1, s).to(skip.dtype)


def install_freeu(oracle_unet, s1: float, s2: float, b1: float, b2: float):
    """Give the first two up blocks of an ``oracle.sd15.UNet2DConditionModel`` a forward that applies FreeU before their ``torch.cat``
    (a method bound on the instance; ``uninstall_freeu`` removes it)."""
    for i in (0, 1):
        blk = oracle_unet.up_blocks[i]

        def forward(self, x, skips, temb, ehs, cak, _i=i):
            for j, r in enumerate(self.resnets):
                x, s = apply_freeu_ref(_i, x, skips.pop(), s1, s2, b1, b2)
                x = r(torch.cat([x, s], dim=1), temb)
                if self.has_attn:
                    x = self.attentions[j](x, ehs, cak)
            if self.add_up:
                x = self.upsamplers[0](x)
            return x
        blk.forward = types.MethodType(forward, blk)
    return oracle_unet


def uninstall_freeu(oracle_unet):
    for i in (0, 1):
        oracle_unet.up_blocks[i].__dict__.pop("forward", None)
    return oracle_unet


def f32(v: float) -> float:
    """The value the C entry point receives for a Python float (its scale arguments are fp32)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- the launch, NHWC -----------------------------------------------------------------------------------------------------------------------------
def concat_freeu_ref(a, b, b_add, backbone_scale, skip_scale, dtype, *, closed=False, anti=False, double=False, drop_add=False, upper=False,
                     filter_backbone_channel=None, skip_unfiltered=None):
    """a [B, H, W, Ca], b / b_add [B, H, W, Cb] holding ``dtype``-representable values -> (float64 [B, H, W, Ca + Cb] BEFORE the final
    rounding, v float64).  v = round16(fp32(b) + fp32(b_add)) as ``imd_concat2`` forms it.  The FFT form unless ``closed`` or a wave
    mutation asks for the closed form.  Mutations (tests/test_freeu_host.py): ``drop_add``; ``upper`` (the upper backbone half scaled);
    ``filter_backbone_channel`` = c (backbone channel c filtered); ``skip_unfiltered`` = c (skip channel c passed through)."""
    a, b = a.to(F64), b.to(F64)
    Ca = a.shape[-1]
    v = b if (b_add is None or drop_add) else (b.float() + b_add.float()).to(dtype).to(F64)
    maps = v.permute(0, 3, 1, 2)
    filt = closed_form(maps, skip_scale, anti=anti, double=double) if (closed or anti or double) else fourier_filter_ref(maps, 1, skip_scale)
    filt = filt.permute(0, 2, 3, 1).contiguous()
    if skip_unfiltered is not None:
        filt[..., skip_unfiltered] = v[..., skip_unfiltered]
    back = a.clone()
    half = slice(Ca // 2, Ca) if upper else slice(0, Ca // 2)
    back[..., half] = back[..., half] * backbone_scale
    if filter_backbone_channel is not None:
        c = filter_backbone_channel
        back[..., c] = fourier_filter_ref(back[..., c], 1, skip_scale)
    return torch.cat([back, filt], -1), v


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------------
EXACT_SKIP_SCALE, EXACT_BACKBONE_SCALE = 0.5, 1.5
EXACT_MAPS = [(4, 4), (2, 4), (2, 2), (1, 2), (1, 1)]
EXACT_LAYOUTS = [(16, 16, 4), (32, 16, 4)]       # (Ca, Cb, G); (32, 16, 4): 12 channels per group -- vectors straddle groups, group 2 (24 .. 35) the backbone / skip boundary, group 1 (12 .. 23) the half boundary
AWKWARD = (2, 2, 1280, 640, 32)                  # (H, W, Ca, Cb, G): the third resnet of up_blocks[1], kept tiny -- 60 channels per group


def exact_cases():
    """(B, H, W, Ca, Cb, G, ctrl)"""
    out = []
    for B in (1, 3):
        for ctrl in (False, True):
            for H, W in EXACT_MAPS:
                for Ca, Cb, G in EXACT_LAYOUTS:
                    out.append((B, H, W, Ca, Cb, G, ctrl))
            out.append((B,) + AWKWARD + (ctrl,))
    return out


def _ternary(g, shape):
    return (torch.randint(-1, 2, shape, generator=g) * 2).to(F64)


def exact_operands(case, seed=0):
    """-> (a, b, b_add or None) float64 with values in {-2, 0, 2}"""
    B, H, W, Ca, Cb, G, ctrl = case
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * W + Ca + 7 * B + int(ctrl))
    a, b = _ternary(g, (B, H, W, Ca)), _ternary(g, (B, H, W, Cb))
    return a, b, (_ternary(g, (B, H, W, Cb)) if ctrl else None)


def snap16(ref: torch.Tensor) -> torch.Tensor:
    """The float64 FFT result of an exact case, snapped to the multiple of 1/16 it is (asserted: within 1e-9 of one)."""
    r = (ref * 16).round()
    assert float((ref * 16 - r).abs().max()) < 1e-9, "an exact case whose output is no multiple of 1/16"
    return r / 16


def exact_expected(case, a, b, b_add, dtype, **mutation):
    ref, _ = concat_freeu_ref(a, b, b_add, EXACT_BACKBONE_SCALE, EXACT_SKIP_SCALE, dtype, **mutation)
    return snap16(ref)


def indicator_maps():
    """name -> (4 x 4 map with values in {-2, 0, 2}, the factor fourier_filter(scale 0.5) multiplies it by)"""
    n = torch.arange(4, dtype=F64)[:, None]
    m = torch.arange(4, dtype=F64)[None, :]
    quarter = lambda k: torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=F64)[(k % 4).long()]      # noqa: E731   cos(2 pi k / 4), exactly
    return {"constant": (torch.full((4, 4), 2.0, dtype=F64), 0.5),
            "diagonal": (2 * quarter(n + m), 0.75),
            "anti-diagonal": (2 * quarter(n - m + 4), 1.0),
            "row-wave": (2 * quarter(m + 0 * n), 0.75)}


def ulp_at(ref: torch.Tensor, dtype) -> torch.Tensor:
    """One unit in the last place of ``dtype`` at the magnitude of every element of ``ref`` (tests/exact_cases.py::ulp_at)."""
    bits = 8 if dtype == torch.bfloat16 else 11
    _, e = torch.frexp(ref.to(F64).abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones_like(ref, dtype=F64), e - bits)
