"""Shared data of the inpainting crop / overlay tests (tests/test_inpaint_crop.py, tests/test_inpaint_overlay_gpu.py): the pinned crop
boxes, mask builders and the arrangement of every (orig, gen, mask) byte triple."""
import numpy as np

# (name, (H, W), rectangle rows t:b cols l:r, extra pixels [(row, col, value)], pad, (processing width, height), box (x1, y1, x2, y2))
BOX_CASES = [
    ("A", (111, 150), (30, 80, 40, 110), [], 8, (128, 128), (32, 12, 118, 98)),
    ("B", (111, 150), (30, 80, 40, 110), [], 0, (128, 128), (40, 20, 110, 90)),
    ("C", (111, 150), (5, 60, 100, 150), [], 8, (128, 128), (82, 0, 150, 68)),
    ("D", (111, 150), (20, 100, 60, 80), [], 4, (128, 128), (26, 16, 114, 104)),
    ("E", (111, 150), (0, 111, 0, 150), [], 16, (128, 128), (0, 0, 150, 111)),
    ("F", (111, 150), (30, 80, 40, 110), [], 8, (96, 128), (32, 0, 118, 111)),
    ("G", (131, 97), (40, 41, 50, 51), [], 3, (128, 128), (47, 37, 54, 44)),
    ("H", (111, 150), (30, 80, 40, 110), [(100, 3, 1)], 8, (128, 128), (0, 0, 118, 111)),
]


def case(name):
    return [c for c in BOX_CASES if c[0] == name][0]


def rect_mask(hw, rect, extra=()):
    m = np.zeros(hw, np.uint8)
    t, b, l, r = rect
    m[t:b, l:r] = 255
    for y, x, v in extra:
        m[y, x] = v
    return m


def case_mask(name):
    c = case(name)
    return rect_mask(c[1], c[2], c[3])


def soft_mask(hw, rect, seed):
    """a feathered mask: 255 inside the rectangle, zero far outside, every grey level in a noisy band around it"""
    rng = np.random.default_rng(seed)
    m = rect_mask(hw, rect).astype(np.int32)
    t, b, l, r = rect
    band = np.zeros(hw, bool)
    band[max(t - 6, 0):b + 6, max(l - 6, 0):r + 6] = True
    band[t + 6:max(b - 6, t + 6), l + 6:max(r - 6, l + 6)] = False
    noise = rng.integers(-64, 320, size=hw).clip(0, 255)          # (0 and 255 are frequent)
    return np.where(band, noise, m).astype(np.uint8)


def noise_image(seed, hw, channels=3):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(hw) + ((channels,) if channels else ()), dtype=np.uint8)


def all_triples():
    """(orig [4096, 4096, 3], gen [4096, 4096, 3], mask [4096, 4096]) uint8: pixel p has mask p & 255, and with q = p >> 8 channel 0
    holds (orig, gen) = (q >> 8, q & 255) -- every one of the 256^3 triples -- channels 1 and 2 two other bijections of q"""
    p = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    m = (p & 255).astype(np.uint8)
    hi, lo = ((p >> 16) & 255).astype(np.uint8), ((p >> 8) & 255).astype(np.uint8)
    orig = np.stack([hi, lo, 255 - hi], -1)
    gen = np.stack([lo, hi, lo ^ 0x55], -1)
    return orig, gen, m


def composite_formula(orig, gen, m):
    """the issue's formula per byte, in numpy"""
    o, g, m = orig.astype(np.uint32), gen.astype(np.uint32), np.asarray(m).astype(np.uint32)
    t = o * (255 - m) + g * m + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def make_inpaint_condition(img_r, m_r):
    """the inpainting script's condition on an already resized uint8 pair: image / 255 with -1 where mask / 255 > 0.5 -> fp32 [H, W, 3]"""
    image = np.array(img_r).astype(np.float32) / 255.0
    image_mask = np.array(m_r).astype(np.float32) / 255.0
    assert image.shape[0:1] == image_mask.shape[0:1]
    image[image_mask > 0.5] = -1.0
    return image
