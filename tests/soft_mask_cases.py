"""Shared data of the soft_mask tests: the window -> latent shapes and step counts of the definition, mask builders, the brute-force
statement of the release step (no closed form, no prefix sums) and the blend masks M_k."""
import numpy as np

# (window H0 x W0) -> (latent h x w)
SHAPES = [((64, 64), (8, 8)), ((100, 77), (8, 8)), ((37, 29), (8, 16)), ((5, 5), (8, 8)), ((768, 1024), (80, 64))]
STEPS = [1, 2, 3, 7, 20, 50, 1000]


def ramp_mask(hw, seed=0):
    """every gray level, in a diagonal ramp with a little noise: uint8 [H0, W0]"""
    H0, W0 = hw
    y, x = np.mgrid[0:H0, 0:W0]
    base = (y * 255 // max(H0 - 1, 1) + x * 255 // max(W0 - 1, 1)) // 2
    noise = np.random.default_rng(seed).integers(-20, 21, size=hw)
    return (base + noise).clip(0, 255).astype(np.uint8)


def noise_mask(hw, seed=0):
    """uniform bytes with 0 and 255 frequent (whole bins of either appear at the small shapes)"""
    return np.random.default_rng(seed).integers(-128, 384, size=hw).clip(0, 255).astype(np.uint8)


def bins(n_in, n_out):
    """[(start, end)] of torch's adaptive_avg_pool2d along one axis, by the floor / ceil definition in exact rationals"""
    from fractions import Fraction
    from math import ceil, floor
    return [(floor(Fraction(i * n_in, n_out)), ceil(Fraction((i + 1) * n_in, n_out))) for i in range(n_out)]


def bin_sums(mask, h, w):
    """(S, cnt) int64 [h, w] each, one Python loop per latent pixel"""
    rows, cols = bins(mask.shape[0], h), bins(mask.shape[1], w)
    S, cnt = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for y, (y0, y1) in enumerate(rows):
        for x, (x0, x1) in enumerate(cols):
            S[y, x] = int(mask[y0:y1, x0:x1].astype(np.int64).sum())
            cnt[y, x] = (y1 - y0) * (x1 - x0)
    return S, cnt


def release_brute(S, cnt, n):
    """the definition: the smallest k with S n > D (n - 1 - k), and n if there is none (S = 0) -- a search over every k, int64 (the
    products stay below 2^40 at the shapes of this file)"""
    S, D = S.astype(np.int64), 255 * cnt.astype(np.int64)
    out, found = np.full(S.shape, n, np.int64), np.zeros(S.shape, bool)
    for k in range(n):
        hit = ~found & (S * n > D * (n - 1 - k))
        out[hit] = k
        found |= hit
    return out


def blend_masks(release, n):
    """M_k = [k >= release] for k = 0 .. n - 1: bool [n, ...]"""
    k = np.arange(n).reshape((n,) + (1,) * release.ndim)
    return k >= release[None].astype(np.int64)


def aligned_binary_mask(hw, latent, on):
    """a {0, 255} mask whose edges lie on bin borders: latent pixels on[y, x] (bool [h, w]) fully 255, the others fully 0; the window
    must be a multiple of the latent on both axes"""
    (H0, W0), (h, w) = hw, latent
    assert H0 % h == 0 and W0 % w == 0
    return np.kron(on.astype(np.uint8) * 255, np.ones((H0 // h, W0 // w), np.uint8))


def three_level_mask(hw, latent, gray):
    """0 / ``gray`` / 255 in three vertical bands of whole latent columns -> (mask uint8 [H0, W0], level index [h, w] in {0, 1, 2})"""
    (H0, W0), (h, w) = hw, latent
    assert H0 % h == 0 and W0 % w == 0 and w >= 3
    level = np.zeros((h, w), np.int64)
    level[:, w // 3:2 * w // 3] = 1
    level[:, 2 * w // 3:] = 2
    values = np.array([0, gray, 255], np.uint8)
    return np.kron(values[level], np.ones((H0 // h, W0 // w), np.uint8)), level
