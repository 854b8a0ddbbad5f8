"""Image pre- and post-processing on the device, bit-exact with Pillow.

Pillow's 8-bit resampler (libImaging/Resample.c) is integer arithmetic once its coefficient table exists: per axis
``out = clip8((2^21 + sum_j in[xmin + j] * k[j]) >> 22)``, horizontal pass first, the vertical pass over the uint8 result of the
horizontal one.  ``resample_tables`` builds the table in float64 exactly as Pillow does; ``imd_image_resample`` (csrc/image.hip)
applies it on the GPU and fuses what follows the resize on the host today -- crop, /255, normalisation, the NCHW / NHWC8 layout.
``resample_reference`` is the same integer formula in numpy (tests, tools/make_image_goldens.py).

``get_crop_region`` (``padding_mask_crop`` of the inpainting pipeline), ``overlay_host`` / ``overlay_reference`` and
``inpaint_condition_host`` are the host side of the inpainting front and back end; ``DeviceImageProcessor.overlay`` /
``.inpaint_condition`` give the same bytes from the GPU (``imd_image_overlay``, ``imd_image_inpaint_condition``).

``mask_filter_host`` is the host side of the inpainting pipeline's ``mask_dilate`` / ``mask_blur`` (``ImageFilter.MaxFilter`` then
``ImageFilter.GaussianBlur`` on the "L" mask); ``gaussian_box`` gives the three integers of Pillow's extended box blur (float32, as
libImaging/BoxBlur.c), ``blur_reference`` / ``dilate_reference`` restate both filters in numpy, and ``DeviceImageProcessor.mask_filter``
gives Pillow's bytes from the GPU (``imd_image_mask_filter``, csrc/image_filter.hip).  Pinned against Pillow ``PILLOW_PINNED``.

``DeviceImageProcessor`` is what the pipelines use after ``enable_device_image_io()``: the only host work left per image is
``convert("RGB" | "L")``, one copy of the uint8 pixels into pinned memory and their upload; the decoder's output comes back as ONE uint8 copy instead of fp32 NCHW.
"""
from __future__ import annotations

import collections
import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

PRECISION_BITS = 22                      # 32 - 8 - 2: Pillow's fixed-point fraction of an 8-bit channel
FILTER_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:           # Keys' cubic, a = -0.5
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:           # sinc(x) sinc(x / 3) on [-3, 3)
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTERS = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


@functools.lru_cache(maxsize=256)
def _tables(n_in: int, n_out: int, filter: str):
    f, S = _FILTERS[filter], FILTER_SUPPORT[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = S * fs
    kmax = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    xmin = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    k = np.zeros((n_out, kmax), np.int32)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        w = [f((j + lo - c + 0.5) * inv) for j in range(hi - lo)]
        ww = 0.0
        for v in w:                          # (summed in tap order, as the C loop does)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[i], count[i] = lo, hi - lo
        for j, v in enumerate(w):
            k[i, j] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    for a in (xmin, count, k):
        a.setflags(write=False)
    return xmin, count, k


def resample_tables(n_in: int, n_out: int, filter: str = "lanczos") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(xmin[n_out], count[n_out], k[n_out][kmax]) int32: the window of source samples each output reads and their fixed-point weights
    (22 fraction bits, rows zero-padded to kmax = 2 ceil(support) + 1), computed in float64 as Pillow's precompute_coeffs /
    normalize_coeffs_8bpc do.  sum |k| * 255 < 2^31 for the three filters, so an int32 accumulator holds the pass.  Cached."""
    if filter not in _FILTERS:
        raise ValueError(f"resample filter must be one of {sorted(_FILTERS)}, got {filter!r}")
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resample_tables: sizes must be positive, got {n_in} -> {n_out}")
    return _tables(int(n_in), int(n_out), filter)


def _pass(a: np.ndarray, table, axis: int) -> np.ndarray:
    xmin, count, k = table
    a = np.moveaxis(a.astype(np.int32), axis, 0)
    out = np.empty((len(xmin),) + a.shape[1:], np.uint8)
    for i in range(len(xmin)):
        n = int(count[i])
        acc = np.tensordot(k[i, :n], a[xmin[i]:xmin[i] + n], axes=(0, 0)).astype(np.int32) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resample_reference(arr: np.ndarray, size: Tuple[int, int], filter: str = "lanczos") -> np.ndarray:
    """``Image.resize`` of uint8 [..., H, W, C] to ``size`` = (height, width) by the integer formula, in numpy: horizontal pass, then the
    vertical pass over its uint8 result; an axis whose size does not change is skipped."""
    arr = np.asarray(arr)
    if arr.dtype != np.uint8 or arr.ndim < 3:
        raise ValueError("resample_reference: uint8 [..., H, W, C] expected")
    H, W = arr.shape[-3], arr.shape[-2]
    if W != size[1]:
        arr = _pass(arr, resample_tables(W, size[1], filter), arr.ndim - 2)
    if H != size[0]:
        arr = _pass(arr, resample_tables(H, size[0], filter), arr.ndim - 3)
    return arr


def tile_rows(table, top: int, rows: int, tile_h: int = ops.IMAGE_TILE_H) -> int:
    """Most source rows that one tile of ``tile_h`` output rows reads, over the tiles of output rows [top, top + rows)"""
    xmin, count, _ = table
    lo = xmin[top:top + rows].astype(np.int64)
    hi = lo + count[top:top + rows]
    starts = range(0, rows, tile_h)
    return int(max(hi[s:s + tile_h].max() - lo[s:s + tile_h].min() for s in starts))


_dev_tables = collections.OrderedDict()     # least recently used first
DEVICE_TABLES_MAX = 64                      # entries kept (a table is n_out * (kmax + 2) int32): bounded like the host cache


def device_tables(n_in: int, n_out: int, filter: str, device) -> dict:
    """The table of one axis on ``device`` (uploaded once per (n_in, n_out, filter, device)) with its host copy"""
    device = torch.device(device)
    key = (n_in, n_out, filter, device.type, device.index)
    t = _dev_tables.get(key)
    if t is None:
        xmin, count, k = resample_tables(n_in, n_out, filter)
        t = dict(host=(xmin, count, k), xmin=torch.from_numpy(xmin.copy()).to(device), count=torch.from_numpy(count.copy()).to(device),
                 k=torch.from_numpy(k.copy()).to(device), kmax=int(k.shape[1]), taps=int(count.max()), n_in=n_in, n_out=n_out)
        _dev_tables[key] = t
        while len(_dev_tables) > DEVICE_TABLES_MAX:
            _dev_tables.popitem(last=False)
    else:
        _dev_tables.move_to_end(key)
    return t


ops._clear_hooks.append(_dev_tables.clear)


def resize_to(src: torch.Tensor, size: Tuple[int, int], filter: str = "lanczos", **stage) -> torch.Tensor:
    """uint8 [B, Hin, Win, C] on the device -> resized to ``size`` = (height, width) and through the output stage of
    ``ops.image_resample`` (kind, a, b, crop, binarize, dtype, out, ...)."""
    Hin, Win = int(src.shape[1]), int(src.shape[2])
    th = device_tables(Win, int(size[1]), filter, src.device) if Win != size[1] else None
    tv = device_tables(Hin, int(size[0]), filter, src.device) if Hin != size[0] else None
    return ops.image_resample(src, (int(size[0]), int(size[1])), th, tv, **stage)


def _is_pil(im) -> bool:
    return hasattr(im, "convert") and hasattr(im, "resize")


def mask_as_l(mask) -> np.ndarray:
    """a mask -- PIL image of any mode, uint8 [H, W], [H, W, 1] or [H, W, 3] -- as "L": uint8 [H, W]"""
    if not _is_pil(mask):
        a = np.asarray(mask)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[-1] not in (1, 3)):
            raise TypeError(f"a mask is a PIL image or a uint8 [H, W], [H, W, 1] or [H, W, 3] array, got {a.dtype} {a.shape}")
        if a.ndim == 2 or a.shape[-1] == 1:
            return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1]))
        from PIL import Image
        mask = Image.fromarray(a)
    return np.asarray(mask.convert("L"))


def get_crop_region(mask, width: int, height: int, pad: int = 0) -> Tuple[int, int, int, int]:
    """diffusers' ``VaeImageProcessor.get_crop_region``: the box (x1, y1, x2, y2) around the non-zero pixels of ``mask`` (a PIL image or
    uint8 array, read as "L"), grown by ``pad`` and then along one axis to the aspect ratio of the processing size ``width`` x
    ``height``, kept inside the image.  An all-zero mask raises ValueError (the library divides by zero there)."""
    m = mask_as_l(mask)
    h, w = m.shape
    cols, rows = np.flatnonzero(m.any(axis=0)), np.flatnonzero(m.any(axis=1))
    if cols.size == 0:
        return crop_region_of_bounds((w, h, -1, -1), w, h, width, height, pad)
    return crop_region_of_bounds((int(cols[0]), int(rows[0]), int(cols[-1]), int(rows[-1])), w, h, width, height, pad)


def crop_region_of_bounds(bounds, w: int, h: int, width: int, height: int, pad: int = 0) -> Tuple[int, int, int, int]:
    """``get_crop_region`` from the box ``bounds`` = (x_min, y_min, x_max, y_max) of the non-zero pixels of a ``w`` x ``h`` mask (what
    ``DeviceImageProcessor.mask_filter(bounds=True)`` reads back); (w, h, -1, -1) is the all-zero mask and raises ValueError."""
    x_min, y_min, x_max, y_max = (int(v) for v in bounds)
    if x_max < 0 or y_max < 0:
        raise ValueError("get_crop_region: the mask is all zero, there is no region to crop to")
    crop_left, crop_right = x_min, w - 1 - x_max
    crop_top, crop_bottom = y_min, h - 1 - y_max
    pad = int(pad)
    x1, y1 = max(crop_left - pad, 0), max(crop_top - pad, 0)
    x2, y2 = min(w - crop_right + pad, w), min(h - crop_bottom + pad, h)
    ratio_crop, ratio_processing = (x2 - x1) / (y2 - y1), width / height
    if ratio_crop > ratio_processing:
        d = int((x2 - x1) / ratio_processing - (y2 - y1))
        y1 -= d // 2
        y2 += d - d // 2
        if y2 >= h:
            diff = y2 - h
            y2 -= diff
            y1 -= diff
        if y1 < 0:
            y2 -= y1
            y1 = 0
        if y2 >= h:
            y2 = h
    else:
        d = int((y2 - y1) * ratio_processing - (x2 - x1))
        x1 -= d // 2
        x2 += d - d // 2
        if x2 >= w:
            diff = x2 - w
            x2 -= diff
            x1 -= diff
        if x1 < 0:
            x2 -= x1
            x1 = 0
        if x2 >= w:
            x2 = w
    return x1, y1, x2, y2


GAUSSIAN_PASSES = 3                      # box blurs per axis of Pillow's GaussianBlur
PILLOW_PINNED = "12.2.0"                 # the Pillow version the blur / maximum restatement was checked against


def gaussian_box(radius: float) -> Tuple[int, int, int]:
    """(r, ww, fw) of ``ImageFilter.GaussianBlur(radius)``: the integers of its extended box blur (libImaging/BoxBlur.c).  The box
    radius is FLOAT32 arithmetic as in the C code (the square root and the floor see double operands, their results are stored as
    float) -- in double precision the integers differ for some radii (0.3 is one).  One pass is then
    ``out[x] = (ww * sum_{j=-r..r} in[c(x+j)] + fw * (in[c(x-r-1)] + in[c(x+r+1)]) + 2^23) >> 24``."""
    radius = float(radius)
    if not math.isfinite(radius) or radius <= 0.0:
        raise ValueError(f"gaussian_box: the radius must be positive and finite, got {radius}")
    f = np.float32
    with np.errstate(over="raise"):
        sigma2 = f(f(f(radius) * f(radius)) / f(GAUSSIAN_PASSES))
        L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
        l = f(math.floor((float(L) - 1.0) / 2.0))
        a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * sigma2)))
        a = f(a / f(f(6) * f(sigma2 - f(f(l + f(1)) * f(l + f(1))))))
        fr = f(l + a)
        r = int(fr)
        ww = int(f(f(1 << 24) / f(f(fr * f(2)) + f(1))))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def _box_pass(a: np.ndarray, box: Tuple[int, int, int]) -> np.ndarray:
    """one extended box blur along the last axis of uint8 ``a``, edges replicated, from an inclusive prefix sum"""
    r, ww, fw = box
    n = a.shape[-1]
    x = np.arange(n)
    v = a.astype(np.uint64)
    P = np.concatenate([np.zeros(a.shape[:-1] + (1,), np.uint64), np.cumsum(v, axis=-1)], axis=-1)          # P[i + 1] = sum in[0..i]
    total = (P[..., np.minimum(x + r, n - 1) + 1] - P[..., np.maximum(x - r - 1, -1) + 1]
             + np.maximum(0, r - x).astype(np.uint64) * v[..., :1] + np.maximum(0, x + r - n + 1).astype(np.uint64) * v[..., -1:])
    edges = v[..., np.clip(x - r - 1, 0, n - 1)] + v[..., np.clip(x + r + 1, 0, n - 1)]
    return ((np.uint64(ww) * total + np.uint64(fw) * edges + np.uint64(1 << 23)) >> np.uint64(24)).astype(np.uint8)


def blur_reference(arr: np.ndarray, radius: float) -> np.ndarray:
    """``Image.filter(ImageFilter.GaussianBlur(radius))`` of uint8 "L" images [..., H, W] by the integer formula, in numpy: three box
    passes along the rows, then three along the columns, each over the uint8 result of the one before.  radius 0 copies."""
    arr = np.asarray(arr)
    if arr.dtype != np.uint8 or arr.ndim < 2:
        raise ValueError("blur_reference: uint8 [..., H, W] expected")
    if float(radius) == 0.0:
        return arr.copy()
    box = gaussian_box(radius)
    for _ in range(GAUSSIAN_PASSES):
        arr = _box_pass(arr, box)
    arr = np.swapaxes(arr, -1, -2)
    for _ in range(GAUSSIAN_PASSES):
        arr = _box_pass(arr, box)
    return np.ascontiguousarray(np.swapaxes(arr, -1, -2))


def dilate_reference(arr: np.ndarray, k: int) -> np.ndarray:
    """``Image.filter(ImageFilter.MaxFilter(2 k + 1))`` of uint8 "L" images [..., H, W] in numpy: the maximum over the
    (2k + 1) x (2k + 1) window clipped at the border, one axis after the other.  k = 0 copies."""
    arr = np.asarray(arr)
    if arr.dtype != np.uint8 or arr.ndim < 2 or int(k) < 0:
        raise ValueError("dilate_reference: uint8 [..., H, W] and k >= 0 expected")
    out = arr.copy()
    for axis in (-1, -2):
        a = np.moveaxis(out, axis, -1)
        n = a.shape[-1]
        res = a.copy()
        for d in range(1, min(int(k), n - 1) + 1):
            res[..., d:] = np.maximum(res[..., d:], a[..., :-d])
            res[..., :-d] = np.maximum(res[..., :-d], a[..., d:])
        out = np.ascontiguousarray(np.moveaxis(res, -1, axis))
    return out


def mask_filter_values(dilate, blur) -> Tuple[int, float]:
    """(dilate, blur) of one mask, checked: a non-negative integer and a non-negative finite radius"""
    if isinstance(dilate, bool) or not isinstance(dilate, (int, np.integer)) or int(dilate) < 0:
        raise ValueError(f"mask_dilate must be a non-negative integer (the window is 2k + 1 pixels), got {dilate!r}")
    if isinstance(blur, bool) or not isinstance(blur, (int, float, np.integer, np.floating)) or not math.isfinite(float(blur)) or float(blur) < 0:
        raise ValueError(f"mask_blur must be a non-negative finite radius, got {blur!r}")
    return int(dilate), float(blur)


def mask_filter_host(mask, dilate: int = 0, blur: float = 0.0):
    """The host route of ``mask_dilate`` / ``mask_blur``: ``mask`` (PIL image of any mode, or a uint8 array) as "L", then
    ``ImageFilter.MaxFilter(2 dilate + 1)`` and ``ImageFilter.GaussianBlur(blur)``; a step whose value is 0 is skipped -> PIL "L" image"""
    from PIL import Image, ImageFilter
    dilate, blur = mask_filter_values(dilate, blur)
    m = mask.convert("L") if _is_pil(mask) else Image.fromarray(mask_as_l(mask))
    if dilate > 0:
        m = m.filter(ImageFilter.MaxFilter(2 * dilate + 1))
    if blur > 0.0:
        m = m.filter(ImageFilter.GaussianBlur(blur))
    return m


def _pool_edges(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """the bins of torch's ``adaptive_avg_pool2d`` along one axis: output i covers [floor(i n_in / n_out), ceil((i + 1) n_in / n_out))"""
    i = np.arange(n_out, dtype=np.int64)
    return i * n_in // n_out, ((i + 1) * n_in + n_out - 1) // n_out


def mask_release_reference(mask_u8: np.ndarray, h: int, w: int, n: int) -> np.ndarray:
    """``soft_mask``: the "L" mask window ``mask_u8`` (uint8 [H0, W0]) -> uint16 [h, w], the step of a run of ``n`` schedule positions
    from which each latent pixel is free to be repainted (Differential Diffusion, Levin & Fried 2023).  Latent pixel (y, x) covers the
    ``adaptive_avg_pool2d`` bin of the window; S = the integer sum of its bytes, D = 255 cnt, c = S / D in [0, 1]:

        release = n - ceil(c n) = n - (S n + D - 1) // D          (64-bit integers: exact)

    so c = 1 gives 0 (repainted at every step), c = 0 gives n (ends as the clean original), and a pixel in between runs its last
    ceil(c n) steps free.  The blend that aims at position k + 1 uses the 0 / 1 mask ``k >= release``.  This is the host route of the
    inpainting pipeline and the oracle of ``DeviceImageProcessor.mask_release`` (``imd_image_mask_release``)."""
    a = np.asarray(mask_u8)
    h, w, n = int(h), int(w), int(n)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"mask_release: the mask window is a non-empty uint8 [H0, W0] array, got {a.dtype} {a.shape}")
    if h < 1 or w < 1:
        raise ValueError(f"mask_release: empty latent ({h} x {w})")
    if not 1 <= n <= 65535:
        raise ValueError(f"mask_release: n must be in [1, 65535], got {n}")
    H0, W0 = a.shape
    (y0, y1), (x0, x1) = _pool_edges(H0, h), _pool_edges(W0, w)
    # prefix sums along the rows (a row of fewer than 2^24 bytes sums below 2^32), the bins' column ranges taken from them, then prefix
    # sums of those [H0, w] column sums down the rows: ONE pass over the window
    P = np.zeros((H0, W0 + 1), dtype=np.uint32 if W0 < (1 << 24) else np.int64)
    np.cumsum(a, axis=1, dtype=P.dtype, out=P[:, 1:])
    Q = np.zeros((H0 + 1, w), dtype=np.int64)
    np.cumsum(P[:, x1].astype(np.int64) - P[:, x0].astype(np.int64), axis=0, out=Q[1:])
    S = Q[y1] - Q[y0]
    D = 255 * ((y1 - y0)[:, None] * (x1 - x0)[None, :])
    return (n - (S * n + D - 1) // D).astype(np.uint16)


def release_of_levels(levels, n: int) -> np.ndarray:
    """``soft_mask`` with ``mask_latents=`` given as a float tensor: levels c in [0, 1] (any shape) -> uint16 release = n - ceil(c n),
    in float64 from the fp32 values.  Non-finite values and values outside [0, 1] raise ValueError."""
    c = (levels.detach().to("cpu", torch.float32).numpy() if isinstance(levels, torch.Tensor) else np.asarray(levels, dtype=np.float32)).astype(np.float64)
    n = int(n)
    if not 1 <= n <= 65535:
        raise ValueError(f"mask_release: n must be in [1, 65535], got {n}")
    if not np.isfinite(c).all() or (c < 0.0).any() or (c > 1.0).any():
        raise ValueError("soft_mask: mask_latents must be finite and in [0, 1]")
    return (n - np.ceil(c * n)).astype(np.uint16)


def overlay_reference(orig: np.ndarray, gen: np.ndarray, mask: np.ndarray, box: Tuple[int, int, int, int]) -> np.ndarray:
    """``Image.composite`` in numpy: uint8 ``orig`` [..., H0, W0, 3], ``mask`` [..., H0, W0], ``gen`` [..., ch, cw, 3] already at the size
    of ``box`` = (x1, y1, x2, y2) -> ``orig`` outside the box, ((t >> 8) + t) >> 8 with t = orig (255 - m) + gen m + 128 inside."""
    x1, y1, x2, y2 = box
    out = np.array(np.broadcast_to(orig, gen.shape[:-3] + orig.shape[-3:]))
    o = out[..., y1:y2, x1:x2, :].astype(np.uint32)
    m = np.asarray(mask)[..., y1:y2, x1:x2, None].astype(np.uint32)
    t = o * (255 - m) + gen.astype(np.uint32) * m + 128
    out[..., y1:y2, x1:x2, :] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def overlay_host(gen: np.ndarray, orig, mask, box: Tuple[int, int, int, int]):
    """The host route of ``overlay=True``: decoded uint8 ``gen`` [H, W, 3] resized to ``box`` = (x1, y1, x2, y2) with Lanczos, pasted
    into a copy of the PIL image ``orig`` ("RGB") and composited with ``orig`` through the PIL mask ``mask`` ("L") -> PIL image"""
    from PIL import Image
    x1, y1, x2, y2 = box
    gen_r = Image.fromarray(gen).resize((x2 - x1, y2 - y1), Image.LANCZOS)
    base = orig.copy()
    base.paste(gen_r, (x1, y1))
    return Image.composite(base, orig, mask)


def inpaint_condition_host(image, mask, box: Optional[Tuple[int, int, int, int]], size: Tuple[int, int]) -> np.ndarray:
    """The inpainting script's ``make_inpaint_condition`` at the processing size: the window ``box`` (None: all) of the PIL ``image``
    ("RGB") and ``mask`` ("L"), each resized with Lanczos to ``size`` = (height, width) -> fp32 [H, W, 3]: image / 255, -1 in the
    three channels where mask / 255 > 0.5."""
    from PIL import Image
    if box is not None:
        image, mask = image.crop(box), mask.crop(box)
    img_r = np.asarray(image.resize((size[1], size[0]), Image.LANCZOS))
    m_r = np.asarray(mask.resize((size[1], size[0]), Image.LANCZOS))
    cond = img_r.astype(np.float32) / 255.0
    cond[m_r.astype(np.float32) / 255.0 > 0.5] = -1.0
    return cond


class DeviceImageProcessor:
    """Image input and output of the pipelines on the GPU.  ``dtype`` is the 16-bit type of the engines (``out="nhwc8"``,
    ``clip_preprocess``)."""

    def __init__(self, device, dtype=torch.float16):
        if dtype not in ops.DTYPE_CODE and dtype != torch.float32:          # (fp32: clip_preprocess and out="nchw" only)
            raise ValueError(f"dtype must be torch.bfloat16, torch.float16 or torch.float32, got {dtype}")
        self.device, self.dtype = torch.device(device), dtype

    # ---- input ----
    def _upload(self, im, mode: str) -> torch.Tensor:
        """one image -> uint8 [1, H, W, C] on the device (PIL / arrays: convert, one copy into pinned memory, one upload)"""
        if isinstance(im, torch.Tensor):
            t = im
        else:
            if _is_pil(im):
                im = im.convert(mode)
            a = np.asarray(im)                 # (a PIL image exports its pixels here; the view is read-only)
            if a.dtype != np.uint8:
                raise TypeError(f"DeviceImageProcessor takes PIL images or uint8 arrays / tensors, got {a.dtype}")
            t = torch.empty(a.shape, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
            np.copyto(t.numpy(), a)            # the one host copy: straight into pinned memory
        if t.dtype != torch.uint8:
            raise TypeError(f"DeviceImageProcessor takes PIL images or uint8 arrays / tensors, got {t.dtype}")
        if t.dim() == 2:
            t = t.unsqueeze(-1)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        want = 3 if mode == "RGB" else 1
        if t.dim() != 4 or t.shape[-1] != want:
            raise ValueError(f"expected uint8 [B, H, W, {want}] (mode {mode}), got {tuple(t.shape)}")
        if not t.is_cuda:
            t = t.contiguous()
            t = (t if t.is_pinned() or self.device.type != "cuda" else t.pin_memory()).to(self.device, non_blocking=True)
        elif t.stride(3) == 1 and t.stride(2) == want:
            return t                           # a window of an uploaded image (rows strided): ``imd_image_resample`` reads it in place
        return t.contiguous()

    @staticmethod
    def _as_list(images) -> list:
        if isinstance(images, (list, tuple)):
            return list(images)
        return [images]

    def preprocess(self, images, size: Optional[Tuple[int, int]] = None, resample: str = "lanczos", out: str = "nhwc8",
                   normalize: bool = True, binarize: bool = False, multiple: int = 8, mode: str = "RGB",
                   _force_two_pass: bool = False) -> torch.Tensor:
        """PIL image(s) or uint8 [B, H, W, C] array(s) / tensor(s) -> ``out="nchw"``: fp32 [B, C, H, W], ``out="nhwc8"``: ``dtype``
        [B, H, W, 8] (channels C..7 zero) -- the values of ``to_image_tensor`` (then ``nchw_to_nhwc8``) bit for bit: resized to
        ``size`` = (height, width) rounded down to a multiple of ``multiple`` with Pillow's ``resample`` filter, /255, and mapped to
        [-1, 1] when ``normalize``.  ``size=None`` keeps each image's size (then they must agree).  ``binarize``: pixels >= 0.5 -> 1, else 0."""
        if out not in ("nhwc8", "nchw"):
            raise ValueError(f"out must be 'nhwc8' or 'nchw', got {out!r}")
        if mode not in ("RGB", "L"):
            raise ValueError(f"mode must be 'RGB' or 'L', got {mode!r}")
        srcs = [self._upload(im, mode) for im in self._as_list(images)]
        if size is not None:
            hw = (int(size[0]) // multiple * multiple, int(size[1]) // multiple * multiple)
        else:
            hw = (int(srcs[0].shape[1]), int(srcs[0].shape[2]))
            if any(tuple(s.shape[1:3]) != hw for s in srcs):
                raise ValueError("preprocess(size=None): the images differ in size")
        C_ = 3 if mode == "RGB" else 1
        B = sum(int(s.shape[0]) for s in srcs)
        if out == "nchw":
            dst = torch.empty(B, C_, hw[0], hw[1], dtype=torch.float32, device=self.device)
            kind = ops.IMAGE_F32_NCHW
        else:
            if self.dtype not in ops.DTYPE_CODE:
                raise ValueError(f"out='nhwc8' needs a 16-bit processor dtype, got {self.dtype}")
            dst = torch.empty(B, hw[0], hw[1], 8, dtype=self.dtype, device=self.device)
            kind = ops.IMAGE_16_NHWC8
        a, b = ((2.0, -1.0) if normalize else (1.0, 0.0))
        i = 0
        for s in srcs:
            n = int(s.shape[0])
            resize_to(s, hw, resample, kind=kind, a=(a,) * 3, b=(b,) * 3, binarize=binarize, out=dst[i:i + n],
                      _force_two_pass=_force_two_pass)
            i += n
        return dst

    def clip_preprocess(self, images, size: int = 224, mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD) -> torch.Tensor:
        """``CLIPImageProcessor()(images).pixel_values`` on the device: bicubic resize of the short edge to ``size`` (long edge
        int(size * long / short)), centre crop, (x / 255 - mean) / std as x / 255 * (1 / std) - mean / std -> [B, 3, size, size] ``dtype``."""
        a = tuple(1.0 / float(s) for s in std)
        b = tuple(-float(m) / float(s) for m, s in zip(mean, std))
        srcs = [self._upload(im, "RGB") for im in self._as_list(images)]
        B = sum(int(s.shape[0]) for s in srcs)
        dst = torch.empty(B, 3, size, size, dtype=torch.float32, device=self.device)
        i = 0
        for s in srcs:
            n, h, w = int(s.shape[0]), int(s.shape[1]), int(s.shape[2])
            short, long_ = (w, h) if w <= h else (h, w)
            new_long = int(size * long_ / short)
            nh, nw = (new_long, size) if w <= h else (size, new_long)
            if nh < size or nw < size:
                raise ValueError(f"clip_preprocess: a {h} x {w} image resizes to {nh} x {nw}, below the {size} x {size} crop")
            resize_to(s, (nh, nw), "bicubic", kind=ops.IMAGE_F32_NCHW, a=a, b=b, crop=((nh - size) // 2, (nw - size) // 2, size, size),
                      out=dst[i:i + n])
            i += n
        return dst if self.dtype == torch.float32 else dst.to(self.dtype)

    def inpaint_condition(self, image, mask, size: Tuple[int, int], box: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
        """``inpaint_condition_host`` on the device: ``image`` (PIL / uint8 [1, H0, W0, 3]) and ``mask`` ("L"; PIL / uint8 [1, H0, W0, 1]),
        their window ``box`` = (x1, y1, x2, y2) resized with Lanczos to ``size`` = (height, width) -> ``dtype`` [1, H, W, 8], the
        16-bit rounding of the host values"""
        img, m = self._upload(image, "RGB"), self._upload(mask, "L")
        if img.shape[:3] != m.shape[:3]:
            raise ValueError(f"inpaint_condition: the image is {tuple(img.shape[1:3])} and the mask {tuple(m.shape[1:3])}")
        if box is not None:
            x1, y1, x2, y2 = box
            img, m = img[:, y1:y2, x1:x2, :], m[:, y1:y2, x1:x2, :]
        return ops.image_inpaint_condition(resize_to(img, size, "lanczos"), resize_to(m, size, "lanczos"), self.dtype)

    def mask_filter(self, mask_u8, dilate: int = 0, blur: float = 0.0, bounds: bool = False, out: Optional[torch.Tensor] = None):
        """``mask_filter_host`` on the device: ``mask_u8`` ("L": PIL / uint8 [H, W], [1 | B, H, W, 1] or an uploaded tensor of that
        shape) through ``ImageFilter.MaxFilter(2 dilate + 1)`` and ``ImageFilter.GaussianBlur(blur)``, Pillow's bytes, a step whose
        value is 0 skipped -> uint8 [B, H, W, 1] on the device.  ``bounds``: -> (mask, int32 [B, 4] on the device) with
        (x_min, y_min, x_max, y_max) of its non-zero pixels, (W, H, -1, -1) when there is none (``crop_region_of_bounds``)."""
        dilate, blur = mask_filter_values(dilate, blur)
        if not isinstance(mask_u8, torch.Tensor) and not _is_pil(mask_u8):
            mask_u8 = mask_as_l(mask_u8)
        m = self._upload(mask_u8, "L")
        src = m[..., 0]
        dst = None if out is None else (out[..., 0] if out.dim() == 4 else out)
        res = ops.image_mask_filter(src, dilate, gaussian_box(blur) if blur > 0.0 else None, out=dst, bounds=bounds)
        if bounds:
            return res[0].unsqueeze(-1), res[1]
        return res.unsqueeze(-1)

    def mask_release(self, mask_u8, h: int, w: int, n: int, box: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
        """``mask_release_reference`` on the device (``imd_image_mask_release``): ``mask_u8`` ("L": PIL / uint8 [H0, W0] or an uploaded
        [1, H0, W0, 1] tensor), its window ``box`` = (x1, y1, x2, y2) (None: the whole mask; the window is a view, nothing is copied)
        -> uint16 [h, w] on the device, the release step of every latent pixel for a run of ``n`` schedule positions."""
        if not isinstance(mask_u8, torch.Tensor) and not _is_pil(mask_u8):
            mask_u8 = mask_as_l(mask_u8)
        m = self._upload(mask_u8, "L")
        if m.shape[0] != 1:
            raise ValueError(f"mask_release: one mask per call, got {tuple(m.shape)}")
        src = m[0, :, :, 0]
        if box is not None:
            x1, y1, x2, y2 = (int(v) for v in box)
            src = src[y1:y2, x1:x2]
        return ops.mask_release(src, h, w, n)

    # ---- output ----
    def overlay(self, decoded: torch.Tensor, orig, mask, box: Tuple[int, int, int, int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``overlay_host`` on the device: uint8 ``decoded`` [B, H, W, 3] (``pack``) resized to ``box`` = (x1, y1, x2, y2) with Lanczos and
        composited into ``orig`` (PIL / uint8 [1 | B, H0, W0, 3]) through ``mask`` ("L"; PIL / uint8 [1 | B, H0, W0, 1]) ->
        uint8 [B, H0, W0, 3] on the device"""
        x1, y1, x2, y2 = (int(v) for v in box)
        gen = resize_to(self._upload(decoded, "RGB"), (y2 - y1, x2 - x1), "lanczos")
        return ops.image_overlay(self._upload(orig, "RGB").contiguous(), self._upload(mask, "L").contiguous(), gen, (x1, y1, x2, y2), out=out)

    def pack(self, nhwc16: torch.Tensor) -> torch.Tensor:
        """decoder output [B, H, W, 4 | 8] 16-bit -> uint8 [B, H, W, 3] on the device"""
        return ops.image_pack_u8(nhwc16)

    def postprocess(self, nhwc16, output_type: str = "pil"):
        """``AutoencoderKL.decode_nhwc`` output (a tensor, or a list of them: VAE slicing) -> ``"np"``: uint8 [B, H, W, 3],
        ``"pil"``: list of images -- the values of the pipelines' host path, through ONE uint8 device-to-host copy."""
        if output_type not in ("np", "pil"):
            raise ValueError(f"postprocess handles output_type 'np' and 'pil', got {output_type!r}")
        parts = [self.pack(y) for y in (nhwc16 if isinstance(nhwc16, (list, tuple)) else [nhwc16])]
        arr = (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy()
        if output_type == "np":
            return arr
        from PIL import Image
        return [Image.fromarray(a) for a in arr]


class MaskProcessor:
    """``pipe.mask_processor``: diffusers' name for the mask side of ``VaeImageProcessor``.  ``blur(image, blur_factor)`` is
    ``image.filter(ImageFilter.GaussianBlur(blur_factor))``: Pillow on the host for a PIL image (its mode kept, as diffusers does), the
    same bytes from the GPU for an uploaded uint8 mask ([H, W], [B, H, W] or [B, H, W, 1] on the device; the shape is kept)."""

    def __init__(self, processor=None):
        self._processor = processor            # () -> DeviceImageProcessor, asked for only when a device tensor comes

    def _device(self, image: torch.Tensor, dilate: int, blur: float) -> torch.Tensor:
        if not image.is_cuda or image.dtype != torch.uint8 or image.dim() not in (2, 3, 4) or (image.dim() == 4 and image.shape[-1] != 1):
            raise TypeError(f"mask_processor takes PIL images or uploaded uint8 [H, W], [B, H, W] or [B, H, W, 1] masks, got "
                            f"{image.dtype} {tuple(image.shape)} on {image.device}")
        proc = self._processor() if self._processor is not None else DeviceImageProcessor(image.device)
        m = image if image.dim() == 4 else (image[None, ..., None] if image.dim() == 2 else image[..., None])
        return proc.mask_filter(m, dilate, blur).reshape(image.shape)

    def blur(self, image, blur_factor: float = 4):
        if isinstance(image, torch.Tensor):
            return self._device(image, 0, mask_filter_values(0, blur_factor)[1])
        from PIL import ImageFilter
        return image.filter(ImageFilter.GaussianBlur(blur_factor))

    def dilate(self, image, k: int = 1):
        """``image.filter(ImageFilter.MaxFilter(2 k + 1))``, host or device as ``blur``"""
        if isinstance(image, torch.Tensor):
            return self._device(image, mask_filter_values(k, 0.0)[0], 0.0)
        from PIL import ImageFilter
        return image.filter(ImageFilter.MaxFilter(2 * int(k) + 1)) if int(k) > 0 else image.copy()


__all__ = ["resample_tables", "resample_reference", "tile_rows", "device_tables", "resize_to", "DeviceImageProcessor", "CLIP_MEAN", "CLIP_STD",
           "get_crop_region", "crop_region_of_bounds", "mask_as_l", "overlay_reference", "overlay_host", "inpaint_condition_host",
           "gaussian_box", "blur_reference", "dilate_reference", "mask_filter_host", "mask_filter_values", "MaskProcessor", "GAUSSIAN_PASSES",
           "PILLOW_PINNED", "mask_release_reference", "release_of_levels"]
