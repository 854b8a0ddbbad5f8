#!/usr/bin/env python
"""Write tests/golden/image_io.npz: what Pillow's ``Image.resize`` and transformers' ``CLIPImageProcessor()`` produce for seeded
uint8 inputs (CPU only).  tests/test_image_tables.py and tests/test_image_io_gpu.py compare the table builder, the integer formula
and the device kernels with these recorded results; neither library is the yardstick at test time.

Contents (``cases`` lists the resample cases as rows Hin, Win, Hout, Wout):
  in_<Hin>x<Win>                      the uint8 [Hin, Win, 3] input of every case with that source size (values are multiples of 17:
                                      16 levels with both extremes, so that the file stays small; C = 1 tests use channel 0)
  out_<i>_<filter>                    ``Image.resize`` of case i, filter in bilinear / bicubic / lanczos (case 5, no resize: the input)
  clip_in_<j>, clip_rows_<j>, clip_lut_<j>, clip_idx_<j>
                                      the key of the input of CLIP case j (the 50 x 37 and the 97 x 131 input above), the rows of the 224 x 224
                                      output that are recorded (every 8th and the last: the resize underneath is checked exactly by
                                      the resample cases, these pin the edge arithmetic, the crop and the normalisation) and
                                      ``CLIPImageProcessor()(image).pixel_values[0][:, rows, :]`` fp32, stored without loss as its
                                      distinct values per channel (lut [3, 256], sorted, NaN padded) and an index map (idx uint8):
                                      pixel_values[c, rows[r], x] = lut[c, idx[c, r, x]] (``clip_pixels`` below)
  pillow_version, transformers_version
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(97, 131, 64, 80),      # non-integer reduction
         (50, 37, 64, 80),       # enlargement (filter scale 1)
         (203, 155, 24, 24),     # strong reduction: ~51 taps with Lanczos
         (64, 80, 64, 48),       # horizontal only
         (64, 80, 40, 80),       # vertical only
         (64, 80, 64, 80)]       # no resize
CLIP_INPUTS = [(50, 37), (97, 131)]
FILTERS = ("bilinear", "bicubic", "lanczos")
CLIP_ROW_STEP = 8
SEED = 20240607
LIMIT = 300 * 1000


def clip_pixels(golden, j: int) -> np.ndarray:
    """the recorded pixel values of CLIP case j: fp32 [3, len(clip_rows_j), 224]"""
    lut, idx = golden[f"clip_lut_{j}"], golden[f"clip_idx_{j}"]
    return np.stack([lut[c][idx[c]] for c in range(3)])


def main():
    import PIL
    from PIL import Image
    import transformers
    from imagdressing_amd.image import resample_reference

    pil_filter = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    rng = np.random.default_rng(SEED)
    data = {"cases": np.asarray(CASES, np.int32), "pillow_version": np.asarray(PIL.__version__),
            "transformers_version": np.asarray(transformers.__version__)}
    for hin, win, _, _ in CASES:
        key = f"in_{hin}x{win}"
        if key not in data:
            data[key] = (rng.integers(0, 16, size=(hin, win, 3)) * 17).astype(np.uint8)
    for i, (hin, win, hout, wout) in enumerate(CASES):
        x = data[f"in_{hin}x{win}"]
        for f in FILTERS:
            ref = np.asarray(Image.fromarray(x).resize((wout, hout), resample=pil_filter[f]))
            mine = resample_reference(x, (hout, wout), f)
            diff = int(np.abs(ref.astype(np.int32) - mine.astype(np.int32)).max())
            print(f"case {i} {hin}x{win} -> {hout}x{wout} {f}: integer formula vs Pillow max |diff| = {diff}")
            if diff != 0:
                raise SystemExit("the integer formula does not reproduce Pillow: fix imagdressing_amd/image.py before recording goldens")
            gray = np.asarray(Image.fromarray(x[..., 0]).resize((wout, hout), resample=pil_filter[f]))
            if not np.array_equal(gray, ref[..., 0]):
                raise SystemExit("Pillow's mode-L result differs from channel 0 of its RGB result")
            if (hin, win) == (hout, wout):
                assert np.array_equal(ref, x)
            else:
                data[f"out_{i}_{f}"] = ref
    proc = transformers.CLIPImageProcessor()
    print("CLIP processor:", type(proc).__name__)
    rows = np.unique(np.r_[np.arange(0, 224, CLIP_ROW_STEP), 223]).astype(np.int32)
    for j, (h, w) in enumerate(CLIP_INPUTS):
        x = data[f"in_{h}x{w}"]
        px = np.asarray(proc(images=Image.fromarray(x), return_tensors="np")["pixel_values"])[0]
        assert px.shape == (3, 224, 224) and px.dtype == np.float32
        px = np.ascontiguousarray(px[:, rows, :])
        lut = np.full((3, 256), np.nan, np.float32)
        idx = np.zeros(px.shape, np.uint8)
        for c in range(3):
            vals, inv = np.unique(px[c], return_inverse=True)
            assert len(vals) <= 256, "more distinct values than uint8 pixels can produce"
            lut[c, :len(vals)], idx[c] = vals, inv.reshape(px[c].shape)
        data[f"clip_in_{j}"], data[f"clip_rows_{j}"], data[f"clip_lut_{j}"], data[f"clip_idx_{j}"] = np.asarray(f"in_{h}x{w}"), rows, lut, idx
        assert np.array_equal(clip_pixels(data, j), px)
    out = os.path.join(ROOT, "tests", "golden", "image_io.npz")
    np.savez_compressed(out, **data)
    size = os.path.getsize(out)
    print(f"wrote {out}: {size} bytes")
    if size > LIMIT:
        raise SystemExit(f"{out} is {size} bytes, over the {LIMIT} byte budget")


if __name__ == "__main__":
    main()
