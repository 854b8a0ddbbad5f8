"""Integer-valued inputs and exact float64 references for the GroupNorm statistics tests (tests/test_gn_exact_inputs.py on the host,
tests/test_gn_statistics_exact_gpu.py on the GPU).  CPU only: torch on the host, nothing of the package is imported here.

Why integers.  Small integers are exact in bf16 up to 256 and in fp16 up to 2048, products of such values are exact in the MFMA, and fp32
sums of integers are exact IN ANY ORDER while every intermediate stays below 2^24.  The tensor a kernel stores and every (sum, sum of squares)
partial it writes are then known exactly, whatever its tiling and summation order: the comparison is ``torch.equal``, and one miscounted
non-zero element anywhere fails it.

Plain tensors (statistics pass, concatenation, consumers): non-zero integers in +-1 .. +-8 plus a per-group integer offset in -3 .. 3 (group
means differ); where the offset cancels a value the value's sign is flipped instead, so no element is zero.  A tiny group whose draw violates
var >= mean^2 gets its signs re-balanced (magnitudes kept).

Convolution operands: x and w in {-2, 0, 2} with density p = min(0.5, sqrt(T / (taps Cin))) -- every product is a multiple of 4, the output's
variance is about 16 T; odd bias, even time-embedding vector, even residual: every output is ODD, hence never zero, and a dropped or doubled
element always changes both S and Q.

Every case must meet PRECONDITIONS (checked by :func:`check_preconditions`; tests/test_gn_exact_inputs.py asserts them for every case)."""
import functools
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
EXACT_BELOW = float(2 ** 24)            # fp32 holds every integer below this

# ---- norm.hip's chunking (gn_pix_per_chunk / gn_chunks) and fold constants, copied so that cases can be chosen on the host; the GPU module checks the
# copy against the library (imd_groupnorm_parts) --------------------------------------------------------------------------------------------------
GN_THREADS, GN_TARGET_BLOCKS, GN_MAX_PPC = 320, 512, 128
GN_TWO_LEVEL_CHUNKS = 256               # more chunks than this: gn_coeffs_kernel + gn_apply_coeffs_kernel
GN_MAX_PARTS = 4096                     # the cap on producer partials per image
GN_FOLD_MAXP = 13                       # partials per thread of the unrolled fold (gn_apply_kernel::MAXP, gemm_common.h::GN_IN_MAXP)


def gn_pix_per_chunk(B: int, HW: int, C: int) -> int:
    vpp = C // 8
    cols = min(vpp, GN_THREADS)
    plan = GN_THREADS // cols
    ppc = (B * HW + GN_TARGET_BLOCKS - 1) // GN_TARGET_BLOCKS
    ppc = (ppc + plan - 1) // plan * plan
    ppc = max(ppc, 2 * plan)
    return min(ppc, GN_MAX_PPC)


def gn_chunks(B: int, HW: int, C: int) -> int:
    ppc = gn_pix_per_chunk(B, HW, C)
    return (HW + ppc - 1) // ppc


def smallest_two_level_hw(B: int, C: int) -> int:
    """The smallest HW at which an ordinary group_norm of [B, HW, C] takes the two-level path (more than GN_TWO_LEVEL_CHUNKS chunks)."""
    hw = 1
    while gn_chunks(B, hw, C) <= GN_TWO_LEVEL_CHUNKS:
        hw += 1
    return hw


# ---- exact statistics ---------------------------------------------------------------------------------------------------------------------------
def group_sums(t: torch.Tensor, G: int):
    """t [B, ..., C] -> (exact float64 [B, G, 2] = (S, Q) per (image, group), n = elements per (image, group))."""
    B, C = t.shape[0], t.shape[-1]
    v = t.to(F64).reshape(B, -1, G, C // G)
    return torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1), v.shape[1] * v.shape[3]


def check_preconditions(out: torch.Tensor, G: int, what: str = "", max_abs: float = 255.0) -> dict:
    """The four conditions a case must meet; raises AssertionError (a case that misses them is an error, never a skip).  -> the figures."""
    sq, n = group_sums(out, G)
    S, Q = sq[..., 0], sq[..., 1]
    fig = dict(max_abs=float(out.abs().max()), zeros=int((out == 0).sum()), q_over_2_24=float(Q.max()) / EXACT_BELOW,
               var_over_mean2=float(((Q * n - S * S) / (S * S).clamp_min(1e-300)).min()), n=n)
    assert torch.equal(out.to(F64), out.to(F64).round()), f"{what}: not integer-valued"
    assert fig["max_abs"] <= max_abs, f"{what}: max |out| = {fig['max_abs']} > {max_abs}"
    assert fig["zeros"] == 0, f"{what}: {fig['zeros']} zeros"
    assert fig["q_over_2_24"] < 1.0, f"{what}: Q reaches 2^24 ({fig['q_over_2_24']:.3f})"
    assert bool((Q * n >= 2 * S * S).all()), f"{what}: var < mean^2 in some (image, group)"
    return fig


# ---- plain tensors ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _rebalance(x: torch.Tensor, G: int) -> torch.Tensor:
    """Re-sign (largest magnitude first, against the running sum) the few (image, group)s whose draw has var < mean^2."""
    B, C = x.shape[0], x.shape[-1]
    cpg = C // G
    v = x.reshape(B, -1, G, cpg).permute(0, 2, 1, 3).reshape(B, G, -1).clone()
    S, Q, n = v.sum(-1), (v * v).sum(-1), v.shape[-1]
    for b, g in (2 * S * S > Q * n).nonzero().tolist():
        vals = v[b, g].abs()
        run = 0.0
        for i in torch.argsort(vals, descending=True).tolist():
            s = -1.0 if run > 0 else 1.0
            run += s * float(vals[i])
            v[b, g, i] = s * vals[i]
    return v.reshape(B, G, -1, cpg).permute(0, 2, 1, 3).reshape(x.shape).contiguous()


def plain_tensor(seed: int, B: int, HW: int, C: int, G: int) -> torch.Tensor:
    """[B, HW, C] float64: non-zero integers, |x| <= 11, group means differ, var >= mean^2 in every (image, group)."""
    g = _gen(seed)
    mag = torch.randint(1, 9, (B, HW, C), generator=g)
    sign = torch.randint(0, 2, (B, HW, C), generator=g) * 2 - 1
    off = torch.randint(-3, 4, (G,), generator=g).repeat_interleave(C // G)
    v = mag * sign
    x = torch.where(v + off == 0, 2 * off, v + off).to(F64)         # (v = -off would give 0: take v = +off)
    return _rebalance(x, G)


# the statistics pass: (B, HW, C, G).  C / G in {4, 8, 10, 12, 24, 40}; G in {8, 16, 24, 32, 64}; C = 2560 (one column pass fills the block);
# C > 2560 (a second column pass: partials accumulate); HW = 1; HW one below / above a multiple of the chunk length (16 pixels at C = 320); B = 3
STATS_PASS_CASES = [
    (3, 37, 128, 32),       # 4 channels per group: every 8-channel vector feeds two groups; B = 3
    (2, 50, 64, 8),         # 8 per group
    (1, 41, 160, 16),       # 10 per group: vectors straddle groups
    (2, 33, 96, 8),         # 12 per group
    (1, 29, 576, 24),       # 24 per group, G = 24
    (2, 19, 2560, 64),      # 40 per group, G = 64, 320 vector columns = the block exactly, one pixel lane
    (1, 7, 2688, 32),       # 336 vector columns: a second column pass (84 per group; group 30 spans both passes)
    (2, 1, 320, 32),        # HW = 1
    (1, 63, 320, 32),       # one pixel short of four 16-pixel chunks
    (1, 65, 320, 32),       # one pixel into the fifth chunk
    (3, 48, 320, 32),       # whole chunks, B = 3
]


def two_level_case():
    """(B, HW, C, G) of the smallest map at C = 128 on which an ordinary call folds through gn_coeffs_kernel + gn_apply_coeffs_kernel."""
    return (1, smallest_two_level_hw(1, 128), 128, 32)


# ---- concatenation ------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, Ca, Cb, G, half, ctrl): ``half`` = the skip tensor holds B / 2 images; ``ctrl`` = the ControlNet addend is present
CONCAT_CASES = [
    (4, 5, 7, 64, 64, 32, True, False),        # 4 channels per group, the skip tensor holds B / 2 images
    (2, 6, 6, 40, 56, 8, False, True),         # 12 per group, Ca = 40: group 3 (channels 36 .. 47) spans both sources; addend
    (2, 8, 8, 320, 320, 32, True, True),       # 20 per group, half + addend
    (3, 3, 11, 24, 136, 16, False, False),     # 10 per group, Ca = 24: group 2 spans both sources, B = 3
]


def concat_operands(seed: int, B: int, H: int, W: int, Ca: int, Cb: int, G: int, half: bool, ctrl: bool, dtype, rounding: bool = False):
    """-> (a [B, H, W, Ca], b [B or B / 2, H, W, Cb], b_add [B, H, W, Cb] or None, expected concatenation [B, H, W, Ca + Cb]), all float64.
    ``rounding`` (with the addend): one or two elements per (image, group) of the skip part sum to an odd integer just ABOVE the element type's
    exact range (bf16: 299, a tie, and 605; fp16: 2049, a tie): the kernel must round the fp32 sum ONCE, to nearest even, and the statistics are
    those of the rounded value.  Such a case exceeds max |out| <= 255 on purpose (the stored values are still exact, Q stays below 2^24)."""
    C = Ca + Cb
    full = plain_tensor(seed, B, H * W, C, G).reshape(B, H, W, C)
    a = full[..., :Ca].contiguous()
    Bb = B // 2 if half else B
    b = full[:Bb, ..., Ca:].contiguous()
    add = None
    if ctrl:
        g = _gen(seed + 1)
        add = (torch.randint(1, 5, (B, H, W, Cb), generator=g) * (torch.randint(0, 2, (B, H, W, Cb), generator=g) * 2 - 1)).to(F64)
        bb = b.repeat(B // Bb, 1, 1, 1)
        add = torch.where(bb + add == 0, -add, add)
        big = () if not rounding else ((192.0, 107.0), (400.0, 205.0)) if dtype == torch.bfloat16 else ((1500.0, 549.0),)
        cpg = C // G
        for gi in range((Ca + cpg - 1) // cpg, G):          # groups that lie wholly in the skip part
            for k, (vb, va) in enumerate(big):
                c = gi * cpg - Ca + (k % cpg)
                pix = (gi * 7 + k * 3) % (H * W)
                b[:, pix // W, pix % W, c] = vb                  # (every image of b: both CFG halves see it)
                add[:, pix // W, pix % W, c] = va
    bb = b.repeat(B // Bb, 1, 1, 1)
    s = bb if add is None else bb + add
    want = torch.cat([a, s.to(dtype).to(F64)], -1)               # the sum is rounded once, to nearest even
    return a, b, add, want


# ---- convolutions -------------------------------------------------------------------------------------------------------------------------------
def _ternary(g, shape, p: float) -> torch.Tensor:
    u = torch.rand(shape, generator=g)
    return torch.where(u < p / 2, -2.0, torch.where(u < p, 2.0, 0.0)).to(F64)


@functools.lru_cache(maxsize=None)
def conv_case(seed: int, B: int, H: int, W: int, Cin: int, Cout: int, stride: int = 1, taps: int = 9, ups: bool = False, T: float = 16.0):
    """-> dict(x [B, H, W, Cin], w [Cout, Cin, k, k], bias [Cout] odd, temb [B, Cout] even, res [B, Ho, Wo, Cout] even,
    out [B, Ho, Wo, Cout] = the exact float64 convolution with the whole epilogue).  Computed once per case and shared: treat as read-only."""
    g = _gen(seed)
    p = min(0.5, math.sqrt(T / (taps * Cin)))
    k = 3 if taps == 9 else 1
    x = _ternary(g, (B, H, W, Cin), p)
    w = _ternary(g, (Cout, Cin, k, k), p)
    bias = (2 * torch.randint(-3, 3, (Cout,), generator=g) + 1).to(F64)            # odd, -5 .. 5
    temb = (2 * torch.randint(-2, 3, (B, Cout), generator=g)).to(F64)              # even, -4 .. 4
    xin = x.permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    conv = F.conv2d(xin, w, None, padding=k // 2, stride=stride).permute(0, 2, 3, 1)
    res = (2 * torch.randint(-3, 4, tuple(conv.shape), generator=g)).to(F64)       # even, -6 .. 6
    out = (conv + bias + temb[:, None, None, :] + res).contiguous()
    return dict(x=x, w=w, bias=bias, temb=temb, res=res, out=out, stride=stride, taps=taps, ups=ups)


# Halo-patch epilogues, un-split: (cfg, B, H, W, Cin, Cout, G, ups).  8 x 16-pixel tiles (5, 22, 29) are ragged in H and W on 12 x 18 and 24 x 40;
# the 16 x 16-pixel tiles of 23 refuse maps lower than 16 rows: ragged on 24 x 40 and 20 x 18.  Cout = 320, G = 32: groups of 10 straddle the 128-channel
# tiles (5, 29) and 8-channel vectors; Cout = 192: neither a multiple of 128 nor of 160.  Config 29 takes Cin % 64 == 0 only.
PATCH_CASES = [(cfg,) + shape + (False,) for cfg, shapes in {
    5: [(2, 12, 18, 64, 320, 32), (1, 24, 40, 64, 320, 32), (2, 16, 16, 96, 128, 8), (2, 16, 16, 64, 192, 8)],
    22: [(2, 12, 18, 64, 320, 32), (1, 24, 40, 64, 320, 32), (2, 16, 16, 96, 128, 8), (2, 16, 16, 64, 192, 8)],
    23: [(2, 20, 18, 64, 320, 32), (1, 24, 40, 64, 320, 32), (2, 16, 16, 96, 128, 8), (2, 16, 16, 64, 192, 8)],
    29: [(2, 12, 18, 64, 320, 32), (1, 24, 40, 64, 320, 32), (2, 16, 16, 64, 192, 8)],
}.items() for shape in shapes] + [
    (5, 1, 6, 9, 64, 128, 8, True),            # the fused nearest-2x upsample (stored map 12 x 18) also hands its statistics on
]

# K slices, statistics from the finish launch: (cfg, B, H, W, Cin, Cout, G, split, stride) -- test_splitk_finish_groupnorm_statistics' configs, batch cut to 2
SPLITK_CASES = [
    (24, 2, 8, 8, 640, 1280, 32, 6, 1),
    (2, 2, 8, 8, 1280, 1280, 32, 6, 1),
    (18, 2, 8, 8, 320, 1280, 32, 3, 1),
    (5, 2, 16, 16, 640, 1280, 32, 4, 1),
    (21, 1, 32, 32, 640, 640, 32, 3, 1),
    (0, 2, 32, 32, 320, 320, 32, 2, 2),        # stride 2
    (2, 3, 8, 8, 128, 96, 8, 2, 1),            # 12 channels per group
    (0, 2, 16, 16, 64, 2560, 32, 2, 1),        # 320 columns: one full pass of the block
]

# Register-staged tiles (GENERIC_GN_STATS): (cfg, B, H, W, Cin, Cout, G, stride, taps, T) -- test_register_staged_tiles_groupnorm_statistics' configs
TILE_CASES = [
    (0, 2, 64, 64, 8, 320, 32, 1, 9, 8.0),     # 40960 elements per group: T = 8 keeps Q below 2^23; the last column tile is half empty
    (-1, 2, 64, 64, 8, 320, 32, 1, 9, 8.0),
    (2, 2, 32, 32, 64, 320, 32, 2, 9, 16.0),   # stride 2, 10 channels per group
    (2, 4, 8, 8, 128, 1280, 32, 1, 1, 16.0),   # 1 x 1 taps
    (1, 2, 16, 16, 64, 192, 8, 1, 9, 16.0),
    (4, 1, 32, 32, 32, 96, 8, 1, 9, 16.0),     # one ragged column tile
    (3, 2, 16, 16, 32, 128, 16, 1, 9, 16.0),
    (7, 2, 16, 16, 32, 128, 16, 1, 1, 16.0),
]

# the eight shapes the construction was first tried on (B, H, W, Cin, Cout, G, stride, T): only 64 x 64 x 1280 (163840 elements per group) needs a small T --
# with this module's epilogue ranges (variance about 36 on top of 16 T) T = 4 still reaches 2^24, T = 2 stays at two thirds of it
TRIED_SHAPES = [
    (2, 12, 18, 64, 320, 32, 1, 16.0), (1, 24, 40, 64, 320, 32, 1, 16.0), (2, 16, 16, 96, 128, 8, 1, 16.0), (2, 8, 8, 1280, 1280, 32, 1, 16.0),
    (2, 16, 16, 640, 1280, 32, 1, 16.0), (2, 32, 32, 320, 320, 32, 2, 16.0), (2, 16, 16, 64, 2560, 32, 1, 16.0), (1, 64, 64, 32, 1280, 32, 1, 2.0),
]


def patch_conv(case):
    cfg, B, H, W, Cin, Cout, G, ups = case
    return conv_case(101, B, H, W, Cin, Cout, 1, 9, ups, 16.0)


def splitk_conv(case):
    cfg, B, H, W, Cin, Cout, G, split, stride = case
    return conv_case(102, B, H, W, Cin, Cout, stride, 9, False, 16.0)


def tile_conv(case):
    cfg, B, H, W, Cin, Cout, G, stride, taps, T = case
    return conv_case(103, B, H, W, Cin, Cout, stride, taps, False, T)


# ---- consumers: crafted partials ----------------------------------------------------------------------------------------------------------------
CONSUMER_GROUPS = (8, 16, 24, 32, 64)


def consumer_nparts(G: int):
    """1 and 2; the two sides of the unrolled fold's limit; the cap."""
    edge = GN_FOLD_MAXP * (GN_THREADS // G)
    return (1, 2, edge, edge + 1, GN_MAX_PARTS)


def consumer_shape(G: int):
    """(B, HW, C) of the small integer tensor the crafted partials describe: 8 channels per group, 37 pixels (three ragged chunks)."""
    return (2, 37, 8 * G)


def consumer_branch(kernel: str, G: int, nparts: int) -> str:
    """The branch of ``kernel`` ('apply' = gn_apply_kernel, 'coeffs' = gn_coeffs_kernel, 'gn_in' = gemm_common.h::gn_in_coeffs) a case exercises."""
    if kernel == "coeffs":
        return "coeffs:loop"
    return f"{kernel}:{'unrolled' if nparts <= GN_FOLD_MAXP * (GN_THREADS // G) else 'loop'}"


CONSUMER_BRANCHES = ("apply:unrolled", "apply:loop", "coeffs:loop", "gn_in:unrolled", "gn_in:loop", "two_level:coeffs+apply_coeffs")
# gn_in_coeffs lives in the row-resident projections: (cfg, K, HW) with HW a multiple of the kernel's row block; the groups K admits
GN_IN_KERNELS = ((12, 320, 128), (13, 640, 128), (14, 1280, 64))
GN_IN_GROUPS = {320: (8, 16, 32, 64), 640: (32,), 1280: (32,)}


def split_partials(seed: int, sums: torch.Tensor, nparts: int) -> torch.Tensor:
    """Exact (S, Q) [B, G, 2] -> integer pieces [B, nparts, G, 2] (float64) that sum to them: random pieces in +-50 (S) / +-500 (Q), a quarter of
    them zero, many negative, the remainder added to one slot.  sum |piece| < 2^24, so EVERY running sum of any fold order is exact in fp32."""
    B, G, _ = sums.shape
    if nparts == 1:
        return sums[:, None].clone()
    g = _gen(seed)
    amp = torch.tensor([50.0, 500.0], dtype=F64)
    pieces = torch.floor((torch.rand((B, nparts, G, 2), generator=g, dtype=F64) * 2 - 1) * amp)
    pieces[torch.rand((B, nparts, G, 1), generator=g).expand(-1, -1, -1, 2) < 0.25] = 0.0
    slot = seed % nparts
    pieces[:, slot] += sums - pieces.sum(1)
    assert torch.equal(pieces.sum(1), sums) and float(pieces.abs().sum(1).max()) < EXACT_BELOW
    return pieces


def gn_reference(x: torch.Tensor, G: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, silu: bool = False):
    """float64 GroupNorm of x [B, HW, C] -> dict(mean, rstd [B, G]; a, b [B, C] with y = x a + b; y [B, HW, C])."""
    sq, n = group_sums(x, G)
    cpg = x.shape[-1] // G
    mean = sq[..., 0] / n
    var = sq[..., 1] / n - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps)
    a = gamma.to(F64) * rstd.repeat_interleave(cpg, 1)
    b = beta.to(F64) - mean.repeat_interleave(cpg, 1) * a
    y = x.to(F64) * a[:, None] + b[:, None]
    if silu:
        y = y * torch.sigmoid(y)
    return dict(mean=mean, rstd=rstd, a=a, b=b, y=y, mean_a=mean.repeat_interleave(cpg, 1) * a)


def ulp_at(ref: torch.Tensor, dtype) -> torch.Tensor:
    """One unit in the last place of ``dtype`` (bf16: 8 significant bits, fp16: 11) at the magnitude of every element of ``ref``."""
    bits = 8 if dtype == torch.bfloat16 else 11
    _, e = torch.frexp(ref.to(F64).abs().clamp_min(2.0 ** -14))      # |ref| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=F64), e - bits)


def away_from_zero_affine(seed: int, C: int):
    """(gamma, beta) fp32 for the 16-bit OUTPUT bar: |gamma| in 0.5 .. 1.5 with both signs, |beta| in 4.5 .. 5.5 with both signs.  The integer
    data normalises to |x^| < 3, so |y| > 0.4 everywhere: y = x a + b never cancels to a value whose 16-bit ulp is below the fp32 arithmetic's own
    error (about 1e-6 |b|) -- a one-ulp bar at the reference's magnitude is then a bar on the kernel, not on fp32."""
    g = _gen(seed)
    sg = torch.randint(0, 2, (C,), generator=g) * 2.0 - 1
    sb = torch.randint(0, 2, (C,), generator=g) * 2.0 - 1
    return (sg * (0.5 + torch.rand(C, generator=g))).float(), (sb * (4.5 + torch.rand(C, generator=g))).float()


# ---- the comparison of the GPU module, and the three mutations it must catch -----------------------------------------------------------------------
def partials_match(partials: torch.Tensor, exact: torch.Tensor) -> bool:
    """THE comparison: partials [B, nparts, G, 2] folded in float64 equal the exact [B, G, 2] sums."""
    return torch.equal(partials.to(F64).sum(1).cpu(), exact)


def mutate_drop(part: torch.Tensor, b: int, g: int, v: float, slot: int = 0) -> torch.Tensor:
    m = part.clone()
    m[b, slot, g, 0] -= v
    m[b, slot, g, 1] -= v * v
    return m


def mutate_double(part: torch.Tensor, b: int, g: int, v: float, slot: int = 0) -> torch.Tensor:
    m = part.clone()
    m[b, slot, g, 0] += v
    m[b, slot, g, 1] += v * v
    return m


def mutate_move(part: torch.Tensor, b: int, g: int, g_to: int, vals: torch.Tensor, slot: int = 0) -> torch.Tensor:
    """Credit the elements ``vals`` of group g (one channel at one pixel, or a whole channel) to group ``g_to``."""
    m = part.clone()
    s, q = float(vals.sum()), float((vals * vals).sum())
    m[b, slot, g, 0] -= s
    m[b, slot, g, 1] -= q
    m[b, slot, g_to, 0] += s
    m[b, slot, g_to, 1] += q
    return m
