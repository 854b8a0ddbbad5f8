"""Shared cases of the per-request ControlNet scale tests (imd_residual_scale_rows and the rows route): the CPU expression that IS the
kernel's contract, the segment shapes, the buffers with sentinels, and the hand-written route table.  No GPU is touched on import."""
import torch

DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))
SENTINEL = 64                  # sentinel elements on either side of every segment
OFFSET = 8                     # a segment's base: 16 bytes past a 256-byte allocation boundary, no more


def oracle(x: torch.Tensor, s: float) -> torch.Tensor:
    """the whole contract of a scaled row, on the CPU: widen, one fp32 multiply, round to nearest even"""
    return (x.float() * torch.tensor(s, dtype=torch.float32)).to(x.dtype)


def expected(x: torch.Tensor, scales) -> torch.Tensor:
    """[rows, ...] on the CPU -> what the launch leaves: a row at exactly 1.0 keeps its bits"""
    out = x.clone()
    for r, s in enumerate(scales):
        if float(s) != 1.0:
            out[r] = oracle(x[r], float(s))
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """distance in units in the last place between two finite 16-bit tensors of one dtype: the difference of their positions in the
    ordered sequence of representable values (sign-magnitude bits -> a monotone integer), which is the ulp at the larger magnitude"""
    def order(t):
        i = bits(t).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)
    return (order(a) - order(b)).abs()


# ---- kernel shapes ----
ONE = (8,)
SIXTEEN = tuple(8 * k for k in (1, 3, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047, 2049))


def residual_row_elems(h: int, w: int, widths=(320, 640, 1280, 1280), layers: int = 2):
    """elements per batch row of the ControlNet residuals of an h x w latent: conv_in, ``layers`` per level, a downsample between
    levels, and the mid block -- 13 at SD1.5 widths"""
    out, hh, ww = [h * w * widths[0]], h, w
    for lv, c in enumerate(widths):
        out += [hh * ww * c] * layers
        if lv < len(widths) - 1:
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            out.append(hh * ww * c)
    out.append(hh * ww * widths[-1])
    return tuple(out)


SD15_8x8 = residual_row_elems(8, 8)
assert len(SD15_8x8) == 13 and SD15_8x8[0] == 64 * 320 and SD15_8x8[-1] == 1280
assert sum(residual_row_elems(64, 80)) * 2 == 16793600          # bytes per batch row at a 512 x 640 image: the bench's traffic figure


def host_segments(row_elems, rows, dtype, seed=0, special=None):
    """-> [(flat CPU buffer, first element, row_elems)] per segment: Gaussian data of ``dtype`` between two runs of SENTINEL elements,
    the whole thing OFFSET elements into its buffer.  ``special``: values written over the head of every row's data."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, n in enumerate(row_elems):
        buf = torch.full((OFFSET + 2 * SENTINEL + rows * n,), -7.0).to(dtype)
        data = (torch.randn(rows, n, generator=g) * 2.0).to(dtype)
        if special is not None:
            m = min(n, special.numel())
            data[:, :m] = special[:m].to(dtype)
        buf[OFFSET + SENTINEL:OFFSET + SENTINEL + rows * n] = data.reshape(-1)
        out.append((buf, OFFSET + SENTINEL, n))
    return out


def segment_views(buffers, rows):
    """the [rows, n] segment tensors inside ``buffers`` (host or device alike)"""
    return [buf[first:first + rows * n].view(rows, n) for buf, first, n in buffers]


# ---- the hand-written route case: R = 3, 10 steps ----
ROUTE_TRIPLES = ((1.0, 0.0, 1.0), (0.5, 0.2, 1.0), (0.8, 0.0, 0.5))
ROUTE_STEPS = 10
ROUTE_ROWS = ([1.0] * 10,
              [0.0, 0.0] + [0.5] * 8,
              [0.8] * 5 + [0.0] * 5)
