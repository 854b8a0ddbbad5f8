"""Reading tests/golden/image_io.npz (written by tools/make_image_goldens.py): the resample cases and the CLIP cases."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bilinear", "bicubic", "lanczos")
# (Hin, Win, Hout, Wout): non-integer reduction, enlargement, strong reduction (~51 Lanczos taps), horizontal only, vertical only, no resize
CASES = [(97, 131, 64, 80), (50, 37, 64, 80), (203, 155, 24, 24), (64, 80, 64, 48), (64, 80, 40, 80), (64, 80, 64, 80)]
CLIP_INPUTS = [(50, 37), (97, 131)]


def load():
    g = np.load(os.path.join(ROOT, "tests", "golden", "image_io.npz"))
    assert [tuple(int(v) for v in row) for row in g["cases"]] == CASES
    return g


def golden_case(g, i, filt):
    """(input uint8 [Hin, Win, 3], Pillow's output uint8 [Hout, Wout, 3]) of case i"""
    hin, win, hout, wout = CASES[i]
    x = g[f"in_{hin}x{win}"]
    return x, (x if (hin, win) == (hout, wout) else g[f"out_{i}_{filt}"])


def clip_case(g, j):
    """(input uint8 [H, W, 3], recorded rows, transformers' pixel values fp32 [3, len(rows), 224]) of CLIP case j"""
    lut, idx = g[f"clip_lut_{j}"], g[f"clip_idx_{j}"]
    return g[str(g[f"clip_in_{j}"])], g[f"clip_rows_{j}"], np.stack([lut[c][idx[c]] for c in range(3)])
