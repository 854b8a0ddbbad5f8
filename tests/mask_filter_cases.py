"""Shared cases of the mask_dilate / mask_blur tests (tests/test_mask_filter_inputs.py, tests/test_mask_filter_gpu.py,
tests/test_mask_blur_pipeline_gpu.py): sizes, radii, window half-widths and image builders.  The yardstick is Pillow itself
(``pillow_filter``); the numpy restatement and the kernel are both compared with it."""
import functools

import numpy as np

SIZES = [(1, 1), (1, 9), (9, 1), (5, 3), (37, 53), (64, 80), (200, 150)]          # (H, W)
RADII = [0.3, 0.5, 1, 1.5, 2, 4, 7.25, 16, 33, 100]
DILATES = [0, 1, 3, 20]
LARGE = ((1024, 768), 33, 8)                                                       # (H, W), radius, k
BATCH = 3
SENTINEL = 0xA5


def images(hw):
    """[(name, uint8 [H, W])]: random bytes, a 255 rectangle on 0, single 255 pixels (corner, edge, centre), all 255, all 0"""
    H, W = hw
    rng = np.random.default_rng(1000 * H + W)
    out = [("random", rng.integers(0, 256, size=hw, dtype=np.uint8))]
    rect = np.zeros(hw, np.uint8)
    rect[H // 4:max(H // 4 + 1, 3 * H // 4), W // 3:max(W // 3 + 1, 2 * W // 3)] = 255
    out.append(("rect", rect))
    for name, (y, x) in (("corner", (0, 0)), ("edge", (H // 2, W - 1)), ("centre", (H // 2, W // 2))):
        p = np.zeros(hw, np.uint8)
        p[y, x] = 255
        out.append((name, p))
    out.append(("ones", np.full(hw, 255, np.uint8)))
    out.append(("zeros", np.zeros(hw, np.uint8)))
    return out


def stack(hw):
    """every image of ``images(hw)`` as one batch: uint8 [7, H, W]"""
    return np.stack([a for _, a in images(hw)])


def pillow_filter(a, k=0, radius=0.0):
    """uint8 [H, W] through Pillow: MaxFilter(2k + 1) when k > 0, then GaussianBlur(radius) when radius > 0"""
    from PIL import Image, ImageFilter
    im = Image.fromarray(np.ascontiguousarray(a))
    assert im.mode == "L"
    if k > 0:
        im = im.filter(ImageFilter.MaxFilter(2 * k + 1))
    if radius > 0:
        im = im.filter(ImageFilter.GaussianBlur(radius))
    return np.array(im)


@functools.lru_cache(maxsize=None)
def _pillow_stack(hw, k, radius):
    out = np.stack([pillow_filter(a, k, radius) for a in stack(hw)])
    out.setflags(write=False)
    return out


def pillow_stack(hw, k=0, radius=0.0):
    """``pillow_filter`` of every image of ``stack(hw)``, computed once and shared (read-only)"""
    return _pillow_stack(tuple(hw), int(k), float(radius))


def nonzero_box(a):
    """(x_min, y_min, x_max, y_max) of the non-zero pixels of uint8 [H, W]; (W, H, -1, -1) when there is none"""
    ys, xs = np.nonzero(a)
    if ys.size == 0:
        return (a.shape[1], a.shape[0], -1, -1)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def strided_batch(hw, seed, row_pad=5, img_pad=3):
    """B = 3 masks inside a buffer filled with SENTINEL: row stride W + row_pad, image stride (H + img_pad) * row stride ->
    (buffer uint8 [B, H + img_pad, W + row_pad], the masks [B, H, W] as a copy)"""
    H, W = hw
    rng = np.random.default_rng(seed)
    buf = np.full((BATCH, H + img_pad, W + row_pad), SENTINEL, np.uint8)
    masks = rng.integers(0, 256, size=(BATCH, H, W), dtype=np.uint8)
    masks[1] = images(hw)[1][1]
    buf[:, :H, :W] = masks
    return buf, masks


# ---- the mistakes the comparison must be able to see (tests/test_mask_filter_inputs.py::test_sensitivity) ----
def box_in_double(radius, passes=3):
    """the box radius computed in double precision"""
    import math
    sigma2 = radius * radius / passes
    L = math.sqrt(12.0 * sigma2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)))
    fr = l + a
    r = int(fr)
    ww = int((1 << 24) / (fr * 2 + 1))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def variant_pass(a, box, pad="edge", use_fw=True, rounding=1 << 23, shift=0):
    """one box pass along the last axis by the direct windowed sum, with a mistake switched on: ``pad="zero"`` pads with zeros instead
    of replicating the edge, ``use_fw=False`` drops the fw term, ``rounding=0`` truncates, ``shift=1`` moves the window by one"""
    r, ww, fw = box
    n = a.shape[-1]
    v = a.astype(np.uint64)
    width = [(0, 0)] * (a.ndim - 1) + [(r + 2, r + 2)]
    p = np.pad(v, width, mode="edge") if pad == "edge" else np.pad(v, width, mode="constant")
    x = np.arange(n) + r + 2 + shift
    total = sum(p[..., x + j] for j in range(-r, r + 1))
    edges = p[..., x - r - 1] + p[..., x + r + 1]
    acc = np.uint64(ww) * total + (np.uint64(fw) * edges if use_fw else 0) + np.uint64(rounding)
    return (acc >> np.uint64(24)).astype(np.uint8)


def variant_blur(a, radius, box=None, passes=3, columns_first=False, **kw):
    box = box or __import__("imagdressing_amd.image", fromlist=["gaussian_box"]).gaussian_box(radius)
    if columns_first:
        a = np.swapaxes(a, -1, -2)
    for _ in range(passes):
        a = variant_pass(a, box, **kw)
    a = np.swapaxes(a, -1, -2)
    for _ in range(passes):
        a = variant_pass(a, box, **kw)
    if not columns_first:
        a = np.swapaxes(a, -1, -2)
    return np.ascontiguousarray(a)
