"""The definition of the device noise source (include/imagdressing_hip.h, imd_noise_params) restated on the CPU: Philox4x32-10 in numpy
unsigned integers, the uniforms and the Box-Muller normals in float64.  Shared by the CPU and the GPU tests; nothing here imports the
package's kernels."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
CLIP = float(np.sqrt(2.0 * np.log(2.0 ** 24)))          # 5.768...: the largest magnitude the definition can give


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 ints -> [..., 4] uint32"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def bits(seed, image, draw, HW):
    """[HW, 4] uint32: the Philox words of every pixel of (seed, image, draw)"""
    pix = np.arange(int(HW), dtype=np.uint64)
    return philox4x32_10((pix, int(image), int(draw), 0), (seed & 0xFFFFFFFF, seed >> 32))


def uniforms(words):
    return ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(seed, image, draw, HW):
    """[HW, 4] float64 standard normals of (seed, image, draw)"""
    u = uniforms(bits(seed, image, draw, HW))
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def nchw(n, h, w):
    """[HW, 4] (the kernel's NHWC pixel order) -> [1, 4, h, w], what the pipelines carry"""
    return np.ascontiguousarray(n.reshape(1, h, w, 4).transpose(0, 3, 1, 2))


# ---- the statistics the issue sets (every figure must be <= 5) ----
STAT_HW = 16384
STAT_SEEDS = (0, 1, 2, 0xFFFFFFFF, 1 << 32, 2 ** 64 - 1, 0x0123456789ABCDEF, 20261020)
STAT_IMAGES = (0, 1)
STAT_DRAWS = (0, 1, 2, 3, 51)
STAT_BAR = 5.0


def corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def tensor_stats(x):
    """the per-tensor figures of one [HW, 4] tensor, each scaled so that 1 is one standard error"""
    x = x.astype(np.float64)
    HW = x.shape[0]
    N = x.size
    m, s = x.mean(), x.std()
    m4 = ((x - m) ** 4).mean() / s ** 4
    out = {"mean": abs(m) * np.sqrt(N), "std": abs(s - 1.0) * np.sqrt(2 * N), "m4": abs(m4 - 3.0) * np.sqrt(N / 96.0)}
    out["channel_pairs"] = max(abs(corr(x[:, a], x[:, b])) for a in range(4) for b in range(a + 1, 4)) * np.sqrt(HW)
    out["lag1"] = max(abs(corr(x[:-1, c], x[1:, c])) for c in range(4)) * np.sqrt(HW)
    return out


def all_stats(get):
    """``get(seed, image, draw)`` -> [STAT_HW, 4]: the worst of every figure over the issue's 80 tensors, and whether all are distinct"""
    t = {(s, i, d): np.asarray(get(s, i, d)) for s in STAT_SEEDS for i in STAT_IMAGES for d in STAT_DRAWS}
    worst = {}

    def take(name, v):
        worst[name] = max(worst.get(name, 0.0), float(v))
    for x in t.values():
        for k, v in tensor_stats(x).items():
            take(k, v)
    rootN = np.sqrt(STAT_HW * 4)
    for s in STAT_SEEDS:
        for d in STAT_DRAWS:
            take("images", abs(corr(t[s, 0, d], t[s, 1, d])) * rootN)
        for i in STAT_IMAGES:
            take("draws", abs(corr(t[s, i, 0], t[s, i, 1])) * rootN)
            take("draws", abs(corr(t[s, i, 2], t[s, i, 3])) * rootN)
    for a, b in zip(STAT_SEEDS, STAT_SEEDS[1:]):          # neighbouring seeds of the list (0/1 and 1/2 differ by one bit pattern step)
        for i in STAT_IMAGES:
            for d in STAT_DRAWS:
                take("seeds", abs(corr(t[a, i, d], t[b, i, d])) * rootN)
    distinct = len({x.tobytes() for x in t.values()}) == len(t)
    return worst, distinct
