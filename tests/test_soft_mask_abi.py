"""C ABI of soft_mask (imd_image_mask_release / imd_soft_mask_rows and their parameter blocks) without a GPU: declared, bound, exported,
named in INTEGRATION.md, the ABI version unchanged (additive), the ctypes mirrors equal to the header field for field, no step
parameter block grown, a foreign struct size refused before any field is read, and every refusal of the launchers, by message -- all
precede the launch."""
import ctypes
import os

import pytest

from tests.test_abi import declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("imd_image_mask_release", "imd_soft_mask_rows")


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def release_block():
    """aligned fake addresses, never dereferenced on the host"""
    from imagdressing_amd import _lib
    p = _lib.ImageMaskReleaseParams()
    p.src, p.src_row_stride, p.out, p.H0, p.W0, p.h, p.w, p.n = 0x1000, 64, 0x2000, 64, 64, 8, 8, 20
    return p


def rows_block():
    from imagdressing_amd import _lib
    p = _lib.SoftMaskRowsParams()
    p.release, p.step_rows, p.mask, p.B, p.HW = 0x1000, 0x2000, 0x3000, 1, 64
    return p


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in declared_functions()
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in text
    assert sorted(_lib.SYMBOLS) == declared_functions()
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert callable(ops.mask_release) and callable(ops.soft_mask_rows)
    assert "soft_mask.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read()


def test_struct_layouts_match_the_header():
    from imagdressing_amd import _lib
    fields = _lib.ImageMaskReleaseParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_image_mask_release_params")
    assert [f[0] for f in fields] == ["struct_bytes", "src", "src_row_stride", "out", "H0", "W0", "h", "w", "n"]
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert kinds["src"] is ctypes.c_void_p and kinds["out"] is ctypes.c_void_p and kinds["src_row_stride"] is ctypes.c_int64
    assert all(kinds[k] is ctypes.c_int for k in ("H0", "W0", "h", "w", "n"))
    fields = _lib.SoftMaskRowsParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_soft_mask_rows_params")
    assert [f[0] for f in fields] == ["struct_bytes", "release", "step_rows", "mask", "B", "HW"]
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert all(kinds[k] is ctypes.c_void_p for k in ("release", "step_rows", "mask"))
    assert kinds["B"] is ctypes.c_int and kinds["HW"] is ctypes.c_int


def test_no_step_block_grew():
    """the mask is written by a launch of its own: the parameter blocks of the eight step entry points are what they were"""
    from imagdressing_amd import _lib
    for cname, py, size, last in (("imd_sampler_params", _lib.SamplerParams, 168, "coefs"), ("imd_unipc_params", _lib.UnipcParams, 184, "coefs"),
                                  ("imd_ddim_params", _lib.DdimParams, 128, "sigma")):
        names = [f[0] for f in py._fields_]
        assert names == header_struct_fields(cname)
        assert names[-1] == last and not any("release" in n or "soft" in n for n in names)
        assert ctypes.sizeof(py) == size, (cname, ctypes.sizeof(py))


@pytest.mark.parametrize("which", [0, 1])
def test_foreign_struct_size_and_null_params_are_refused(lib, which):
    from imagdressing_amd import _lib
    cls, fn, word = ((_lib.ImageMaskReleaseParams, lib.imd_image_mask_release, b"image_mask_release:"),
                     (_lib.SoftMaskRowsParams, lib.imd_soft_mask_rows, b"soft_mask_rows:"))[which]
    p = cls()
    assert p.struct_bytes == ctypes.sizeof(cls)
    for bad in (p.struct_bytes - 8, p.struct_bytes + 8, ctypes.sizeof(_lib.SamplerParams), 0):
        q = cls()
        q.struct_bytes = bad            # every pointer is NULL: a library that read on would answer "null ..." instead
        assert fn(ctypes.byref(q), None) != 0
        assert lib.imd_last_error().startswith(word) and b"parameter block is" in lib.imd_last_error()
    assert fn(None, None) != 0 and word + b" null params" in lib.imd_last_error()
    assert fn(ctypes.byref(p), None) != 0 and word + b" null" in lib.imd_last_error()


RELEASE_REFUSALS = [(dict(src=None), b"null src"), (dict(out=None), b"null out"),
                    (dict(h=0), b"empty latent"), (dict(w=0), b"empty latent"), (dict(h=-1), b"empty latent"),
                    (dict(H0=0), b"empty mask window"), (dict(W0=0), b"empty mask window"), (dict(W0=-3), b"empty mask window"),
                    (dict(src_row_stride=63), b"src_row_stride (63) is below W0 (64)"), (dict(src_row_stride=-64), b"is below W0"),
                    (dict(n=0), b"n (0) must be in [1, 65535]"), (dict(n=65536), b"must be in [1, 65535]"), (dict(n=-5), b"[1, 65535]"),
                    (dict(out=0x2001), b"out must be 2-byte aligned"),
                    (dict(H0=65536, W0=32768, src_row_stride=32768), b"mask window too large")]
ROWS_REFUSALS = [(dict(release=None), b"null release"), (dict(step_rows=None), b"null step_rows"), (dict(mask=None), b"null mask"),
                 (dict(release=0x1002), b"release must be 8-byte aligned"), (dict(release=0x1004), b"8-byte"),
                 (dict(step_rows=0x2002), b"step_rows must be 4-byte aligned"),
                 (dict(mask=0x3004), b"mask must be 16-byte aligned"), (dict(mask=0x3008), b"16-byte"),
                 (dict(B=0), b"empty mask"), (dict(B=-1), b"empty mask"), (dict(HW=0), b"empty mask"), (dict(HW=-7), b"empty mask"),
                 (dict(B=65536), b"at most 65535")]


@pytest.mark.parametrize("case", range(len(RELEASE_REFUSALS)))
def test_release_refusals_precede_the_launch(lib, case):
    over, word = RELEASE_REFUSALS[case]
    p = release_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_image_mask_release(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"image_mask_release:") and word in err and b"launch failed" not in err, err


@pytest.mark.parametrize("case", range(len(ROWS_REFUSALS)))
def test_rows_refusals_precede_the_launch(lib, case):
    over, word = ROWS_REFUSALS[case]
    p = rows_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_soft_mask_rows(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"soft_mask_rows:") and word in err and b"launch failed" not in err, err


def test_the_wrappers_have_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    with pytest.raises(ImdError):
        ops.mask_release(torch.zeros(8, 8, dtype=torch.uint8), 2, 2, 4)
    with pytest.raises(ImdError):
        ops.soft_mask_rows(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.uint16), torch.zeros(2, dtype=torch.int32))
