"""Operands of the exact family of ``imd_lora_expand_rows`` (shared by tests/test_lora_rows_inputs.py, CPU, and
tests/test_lora_rows_gpu.py): x in {-2 .. 2}, `down` rows with at most 32 entries of +-1 (the rest 0), scales in {0, 0.5, 1, 2}.  Every
finished sum is an integer of magnitude <= 64 and every scaled value is representable in bf16 and fp16, so the expected output is known
exactly whatever the summation order -- and an entry index off by one row, a dropped `down` row or a scale on the wrong third of T moves it.

Everything is numpy / float64; nothing here needs a device."""
import numpy as np

# (C, T, E, rows_per_entry): ragged C, the largest T, the real widths, the text + face token count, the smallest C
SHAPES = [(80, 16, 2, 72), (320, 384, 3, 200), (640, 128, 2, 64), (1280, 128, 4, 16), (768, 32, 6, 81), (64, 48, 2, 77),
          # how the launcher deals the T chunks over workgroups depends on the row count: the shapes above give every chunk a workgroup of
          # its own; 100 row blocks x 12 chunks run 4 chunks per workgroup, 194 row blocks walk all their chunks in one
          (320, 384, 2, 3200), (64, 48, 2, 6200)]
SCALES = (0.0, 0.5, 1.0, 2.0)
MAX_NONZERO = 32


def exact_operands(C, T, E, rpe, seed=0):
    """-> x [M, C], down [T, C], scale [E] as float64 arrays of the exact family"""
    rng = np.random.default_rng(1000 * seed + C + 7 * T + E)
    M = E * rpe
    x = rng.integers(-2, 3, size=(M, C)).astype(np.float64)
    down = np.zeros((T, C), dtype=np.float64)
    for j in range(T):
        n = int(rng.integers(8, MAX_NONZERO + 1))
        cols = rng.choice(C, size=min(n, C), replace=False)
        down[j, cols] = rng.choice([-1.0, 1.0], size=cols.size)
    # every scale value occurs when E allows it; neighbouring entries always differ, so an entry index off by one row shows
    scale = np.array([SCALES[(e + 1 + seed) % len(SCALES)] for e in range(E)], dtype=np.float64)
    return x, down, scale


def entry_of_row(M, rpe, shift=0):
    """entry index of every row; ``shift``: the wrong index a kernel would compute from (m + shift) / rows_per_entry"""
    m = np.arange(M) + shift
    return np.clip(m // rpe, 0, M // rpe - 1)


def expected(x, down, scale, rpe, *, entry_shift=0, drop_row=None, group_scales=None):
    """float64 [M, C + T]: the pass-through columns and the scaled tail.  The keyword arguments describe WRONG kernels:
    ``entry_shift`` (entry index from m + shift), ``drop_row`` (that `down` row contributes nothing), ``group_scales`` (a factor per
    third of T on top of the row scale, e.g. (2, 1, 1): a scale applied to the wrong third)."""
    M, C = x.shape
    T = down.shape[0]
    d = down.copy()
    if drop_row is not None:
        d[drop_row] = 0.0
    sums = x @ d.T
    tail = scale[entry_of_row(M, rpe, entry_shift)][:, None] * sums
    if group_scales is not None:
        g = np.repeat(np.asarray(group_scales, dtype=np.float64), T // len(group_scales))
        tail = tail * g[None, :]
    return np.concatenate([x, tail], axis=1)


def representable(v, mant_bits, emin, emax_value):
    """are all float64 values exactly representable in a binary format with ``mant_bits`` explicit mantissa bits, smallest normal
    exponent ``emin`` and largest finite value ``emax_value`` (normals only; 0 counts)"""
    v = np.abs(np.asarray(v, dtype=np.float64)).ravel()
    nz = v[v != 0]
    if nz.size == 0:
        return True
    m, e = np.frexp(nz)                       # nz = m 2^e, m in [0.5, 1)
    scaled = m * 2.0 ** (mant_bits + 1)       # an integer iff mant_bits + 1 significant bits suffice
    return bool(np.all(scaled == np.round(scaled)) and np.all(e - 1 >= emin) and np.all(nz <= emax_value))


def fits_fp16(v):
    return representable(v, 10, -14, 65504.0)


def fits_bf16(v):
    return representable(v, 7, -126, 3.3895313892515355e38)
