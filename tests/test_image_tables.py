"""Image I/O without a GPU: the coefficient tables of imagdressing_amd.image applied with the integer formula reproduce the recorded
Pillow results (tests/golden/image_io.npz, tools/make_image_goldens.py) exactly; table invariants; and the C ABI of
imd_image_resample / imd_image_pack_u8 -- declared, bound, struct mirrors equal to the header, every refusal before any launch."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_abi import declared_functions, header_struct_fields

from tests.image_golden import CASES, FILTERS, ROOT, clip_case, golden_case, load


@pytest.fixture(scope="module")
def golden():
    return load()


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- tables and the integer formula ----
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_integer_formula_equals_recorded_pillow(golden, case, filt):
    from imagdressing_amd.image import resample_reference
    x, want = golden_case(golden, case, filt)
    hout, wout = CASES[case][2:]
    assert want.shape == (hout, wout, 3)
    got = resample_reference(x, (hout, wout), filt)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(resample_reference(x[..., :1], (hout, wout), filt), want[..., :1])          # C = 1: channel 0
    both = resample_reference(np.stack([x, x[::-1].copy()]), (hout, wout), filt)                        # a batch axis in front
    assert np.array_equal(both[0], want)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_integer_formula_equals_live_pillow(golden, case, filt):
    """an additional check where Pillow imports (the recorded results above are the yardstick)"""
    Image = pytest.importorskip("PIL.Image")
    from imagdressing_amd.image import resample_reference
    x, _ = golden_case(golden, case, filt)
    hout, wout = CASES[case][2:]
    live = np.asarray(Image.fromarray(x).resize((wout, hout), resample=getattr(Image, filt.upper())))
    assert np.array_equal(resample_reference(x, (hout, wout), filt), live)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("n_in,n_out", [(131, 80), (37, 80), (155, 24), (203, 24), (80, 48), (64, 40), (1024, 640), (768, 512), (7, 1), (1, 5)])
def test_table_invariants(n_in, n_out, filt):
    from imagdressing_amd.image import FILTER_SUPPORT, resample_tables
    xmin, count, k = resample_tables(n_in, n_out, filt)
    assert xmin.dtype == count.dtype == k.dtype == np.int32
    assert xmin.shape == count.shape == (n_out,) and k.shape[0] == n_out
    kmax = k.shape[1]
    assert kmax == 2 * int(np.ceil(FILTER_SUPPORT[filt] * max(n_in / n_out, 1.0))) + 1
    assert (xmin >= 0).all() and (count >= 1).all() and (xmin + count <= n_in).all() and (count <= kmax).all()
    for i in range(n_out):
        assert (k[i, count[i]:] == 0).all()                                  # zero padded
        assert abs(int(k[i].sum()) - (1 << 22)) <= count[i]                  # weights sum to one up to one rounding per tap
    assert int(np.abs(k).sum(1).max()) * 255 < 2 ** 31                       # the int32 accumulator holds any uint8 input
    assert resample_tables(n_in, n_out, filt)[2] is k                        # cached
    with pytest.raises(ValueError):
        k[0, 0] = 1                                                          # ... and therefore read-only


def test_lanczos_strong_reduction_has_about_51_taps():
    from imagdressing_amd.image import resample_tables
    _, count, k = resample_tables(203, 24, "lanczos")
    assert count.max() in (50, 51, 52) and k.shape[1] == 53


def test_tile_rows():
    from imagdressing_amd import ops
    from imagdressing_amd.image import resample_tables, tile_rows
    t = resample_tables(203, 24, "lanczos")
    xmin, count, _ = t
    want = max(int((xmin[s:s + 8] + count[s:s + 8]).max() - xmin[s:s + 8].min()) for s in range(0, 24, 8))
    assert tile_rows(t, 0, 24) == want and want * ops.IMAGE_TILE_W * 3 <= ops.IMAGE_LDS_BYTES
    assert tile_rows(t, 3, 5) == int((xmin[3:8] + count[3:8]).max() - xmin[3])
    tall = resample_tables(800, 8, "lanczos")
    assert tile_rows(tall, 0, 8) == 800 and 800 * ops.IMAGE_TILE_W * 3 > ops.IMAGE_LDS_BYTES              # the two-launch road


def test_unknown_filter_and_sizes_are_refused():
    from imagdressing_amd.image import resample_tables
    with pytest.raises(ValueError):
        resample_tables(10, 5, "nearest")
    with pytest.raises(ValueError):
        resample_tables(0, 5, "lanczos")


def test_clip_golden_is_the_affine_map_of_the_recorded_resize(golden):
    """the CLIP golden's own consistency: bicubic short-edge resize (integer formula), centre crop, (x / 255 - mean) / std"""
    from imagdressing_amd.image import CLIP_MEAN, CLIP_STD, resample_reference
    for j, (h, w) in enumerate(((50, 37), (97, 131))):
        x, rows, want = clip_case(golden, j)
        assert x.shape == (h, w, 3) and want.shape == (3, len(rows), 224) and rows[0] == 0 and rows[-1] == 223
        nh, nw = (int(224 * h / w), 224) if w <= h else (224, int(224 * w / h))
        r = resample_reference(x, (nh, nw), "bicubic")
        top, left = (nh - 224) // 2, (nw - 224) // 2
        r = r[top:top + 224, left:left + 224][rows]
        mine = (r.astype(np.float64) / 255.0 - np.asarray(CLIP_MEAN)) / np.asarray(CLIP_STD)
        assert np.abs(mine.transpose(2, 0, 1) - want).max() <= 1e-5


# ---- C ABI ----
def test_image_entry_points_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    for name in ("imd_image_resample", "imd_image_resample_form", "imd_image_pack_u8"):
        assert name in declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    text = open(os.path.join(ROOT, "include", "imagdressing_hip.h")).read()
    assert f"IMD_IMG_U8 = {ops.IMAGE_U8}, IMD_IMG_F32_NCHW = {ops.IMAGE_F32_NCHW}, IMD_IMG_16_NHWC8 = {ops.IMAGE_16_NHWC8}" in text
    for name, val in (("IMD_IMG_FORCE_TWO_PASS", ops.IMAGE_FORCE_TWO_PASS), ("IMD_IMG_TILE_W", ops.IMAGE_TILE_W),
                      ("IMD_IMG_TILE_H", ops.IMAGE_TILE_H), ("IMD_IMG_LDS_BYTES", ops.IMAGE_LDS_BYTES)):
        assert f"#define {name} {val}\n" in text
    assert "imd_image_resample" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("cname,pyname", [("imd_image_resample_params", "ImageResampleParams"), ("imd_image_pack_params", "ImagePackParams")])
def test_struct_layout_matches_header(cname, pyname):
    from imagdressing_amd import _lib
    fields = getattr(_lib, pyname)._fields_
    assert [f[0] for f in fields] == header_struct_fields(cname)
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    if pyname == "ImageResampleParams":
        assert kinds["a"] is kinds["b"] is ctypes.c_float * 3
        assert kinds["src_row_stride"] is kinds["src_img_stride"] is ctypes.c_int64
        for ptr in ("src", "out", "tmp", "h_xmin", "h_count", "h_k", "v_xmin", "v_count", "v_k"):
            assert kinds[ptr] is ctypes.c_void_p, ptr
        for name in ("B", "Hin", "Win", "C", "Hres", "Wres", "h_kmax", "h_taps", "v_kmax", "v_taps", "v_tile_rows", "top", "left", "crop_h",
                     "crop_w", "kind", "dtype", "binarize", "flags"):
            assert kinds[name] is ctypes.c_int, name


def launchable_block():
    """97 x 131 x 3 -> 64 x 80, both axes, fp32 NCHW: a block that would launch (addresses are never dereferenced on the host)"""
    from imagdressing_amd import _lib
    p = _lib.ImageResampleParams()
    p.src, p.out, p.tmp = 0x10000, 0x20000, 0x30000
    p.src_row_stride, p.src_img_stride = 131 * 3, 97 * 131 * 3
    p.B, p.Hin, p.Win, p.C, p.Hres, p.Wres = 2, 97, 131, 3, 64, 80
    p.h_xmin, p.h_count, p.h_k, p.h_kmax, p.h_taps = 0x40000, 0x41000, 0x42000, 11, 10
    p.v_xmin, p.v_count, p.v_k, p.v_kmax, p.v_taps = 0x50000, 0x51000, 0x52000, 11, 10
    p.v_tile_rows, p.top, p.left, p.crop_h, p.crop_w = 24, 0, 0, 64, 80
    p.kind = 1
    return p


def test_launchable_block_plans_one_or_two_launches(lib):
    p = launchable_block()
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 1
    p.flags = 1                                                   # IMD_IMG_FORCE_TWO_PASS
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 2
    p.flags, p.v_tile_rows = 0, 32768 // (32 * 3)                 # the most rows the LDS tile holds ...
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 1
    p.v_tile_rows += 1                                            # ... and one more
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 2
    p.C, p.src_row_stride, p.v_tile_rows = 1, 131, 1024
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 1
    p.v_tile_rows = 1025
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 2
    p.h_xmin = p.h_count = p.h_k = None                           # one axis only: always one launch
    p.Wres, p.crop_w = 131, 131
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 1


def test_foreign_struct_size_is_refused(lib):
    from imagdressing_amd import _lib
    for cls, fn, word in ((_lib.ImageResampleParams, lib.imd_image_resample, b"image_resample"),
                          (_lib.ImagePackParams, lib.imd_image_pack_u8, b"image_pack_u8")):
        p = cls()
        assert p.struct_bytes == ctypes.sizeof(cls)
        for bad in (ctypes.sizeof(cls) - 8, ctypes.sizeof(cls) + 8, 0):
            p.struct_bytes = bad            # every pointer is NULL: a library that read on would answer "null pointer" instead
            assert fn(ctypes.byref(p), None) != 0
            assert word in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
        assert fn(None, None) != 0 and b"null params" in lib.imd_last_error()
        q = cls()
        assert fn(ctypes.byref(q), None) != 0 and b"null pointer" in lib.imd_last_error()
    p = launchable_block()
    p.struct_bytes -= 8
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 0


def refusal_cases():
    """(field overrides, words of the error) on top of launchable_block()"""
    return [(dict(src=None), b"null pointer"), (dict(out=None), b"null pointer"),
            (dict(C=2), b"C (2) must be 1 or 3"), (dict(C=4), b"C (4) must be 1 or 3"), (dict(C=0), b"C (0) must be 1 or 3"),
            (dict(top=1), b"crop"), (dict(left=1), b"crop"), (dict(top=-1), b"crop"), (dict(crop_h=65), b"crop"), (dict(crop_w=81), b"crop"),
            (dict(top=60, crop_h=5), b"outside the resized image"), (dict(crop_w=0), b"crop"),
            (dict(h_taps=12), b"horizontal count (12) exceeds kmax (11)"), (dict(v_taps=12), b"vertical count (12) exceeds kmax (11)"),
            (dict(h_kmax=0), b"exceeds kmax"), (dict(kind=3), b"unknown output kind 3"), (dict(kind=-1), b"unknown output kind -1"),
            (dict(kind=2, dtype=7), b"unknown dtype 7"), (dict(kind=2, out=0x20008), b"16-byte"), (dict(out=0x20002), b"4-byte"),
            (dict(h_k=None), b"incomplete horizontal table"), (dict(v_xmin=None), b"incomplete vertical table"),
            (dict(h_xmin=None, h_count=None, h_k=None), b"horizontal axis skipped but the width changes"),
            (dict(v_xmin=None, v_count=None, v_k=None), b"vertical axis skipped but the height changes"),
            (dict(flags=1, tmp=None), b"need the uint8 intermediate"), (dict(v_tile_rows=400, tmp=None), b"need the uint8 intermediate"),
            (dict(v_tile_rows=0, tmp=None), b"need the uint8 intermediate"),
            (dict(src_row_stride=131 * 3 - 1), b"row stride"), (dict(B=0), b"empty image"), (dict(Hres=0), b"empty image")]


@pytest.mark.parametrize("case", range(len(refusal_cases())))
def test_resample_refusals_precede_the_launch(lib, case):
    over, word = refusal_cases()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_image_resample(ctypes.byref(p), None) != 0
    assert word in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error(), lib.imd_last_error()
    assert lib.imd_image_resample_form(ctypes.byref(p)) == 0


@pytest.mark.parametrize("over,word", [(dict(src=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(ld=3), b"ld (3) must be 4 or 8"),
                                       (dict(ld=16), b"ld (16) must be 4 or 8"), (dict(dtype=2), b"unknown dtype 2"), (dict(B=0), b"empty image"),
                                       (dict(src=0x1004), b"8-byte")])
def test_pack_refusals_precede_the_launch(lib, over, word):
    from imagdressing_amd import _lib
    p = _lib.ImagePackParams()
    p.src, p.out, p.B, p.H, p.W, p.ld, p.dtype = 0x1000, 0x2000, 1, 8, 8, 4, 1
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_image_pack_u8(ctypes.byref(p), None) != 0
    assert word in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error(), lib.imd_last_error()


def test_image_ops_have_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    from imagdressing_amd.image import DeviceImageProcessor
    with pytest.raises(ImdError):
        ops.image_resample(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (8, 8), None, None)
    with pytest.raises(ImdError):
        ops.image_pack_u8(torch.zeros(1, 8, 8, 4, dtype=torch.float16))
    with pytest.raises(ValueError):
        DeviceImageProcessor("cpu", torch.float64)


def test_device_image_io_is_off_by_default_and_toggles():
    from imagdressing_amd.dressing_sd.pipelines._base import PipelineBase
    pipe = PipelineBase()
    assert not getattr(pipe, "_device_image_io", False)
    assert pipe.enable_device_image_io() is pipe and pipe._device_image_io is True
    assert pipe.disable_device_image_io() is pipe and pipe._device_image_io is False
    import torch
    x = np.zeros((16, 16, 3), np.uint8)
    t, hw = pipe.enable_device_image_io()._image_tensor([x], "cpu", normalize=True)          # a CPU target keeps the host route
    assert t.shape == (1, 3, 16, 16) and t.dtype == torch.float32 and (t == -1).all() and hw == (16, 16)
