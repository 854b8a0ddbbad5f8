"""C ABI of the per-row residual scale (imd_residual_scale_rows / imd_scale_rows_params) without a GPU: declared, bound, exported, listed
in build.sh, the ABI version unchanged (a new symbol only), the ctypes mirror equal to the header name for name and byte for byte (the
size a C compiler gives the struct), every refusal by name before any launch, and the argument checks of ``ops.residual_scale_rows``."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from tests.test_abi import HEADER, declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "imd_residual_scale_rows"


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    assert NAME in declared_functions()
    assert NAME in _lib.SYMBOLS and hasattr(lib, NAME)
    assert sorted(_lib.SYMBOLS) == declared_functions()
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # a new symbol only: the version stays
    assert callable(ops.residual_scale_rows)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "residual_scale_rows.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read().split()
    assert os.path.isfile(os.path.join(ROOT, "imagdressing_amd", "csrc", "residual_scale_rows.hip"))
    assert "imd_launch_residual_scale_rows" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "imd_kernels.h")).read()


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.ScaleRowsParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_scale_rows_params")
    assert [f[0] for f in fields] == ["struct_bytes", "dtype", "rows", "segments", "scale_rows", "data", "row_elems"]
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert kinds["dtype"] is ctypes.c_int and kinds["rows"] is ctypes.c_int and kinds["segments"] is ctypes.c_int
    assert kinds["scale_rows"] is ctypes.c_void_p
    assert kinds["data"]._length_ == kinds["row_elems"]._length_ == _lib.SCALE_ROWS_MAX_SEGMENTS == 16
    assert kinds["data"]._type_ is ctypes.c_void_p and kinds["row_elems"]._type_ is ctypes.c_int
    assert "#define IMD_SCALE_ROWS_MAX_SEGMENTS 16" in open(HEADER).read()
    # LP64: uint32 + 3 ints, a pointer, 16 pointers, 16 ints -- no padding anywhere
    assert ctypes.sizeof(_lib.ScaleRowsParams) == 16 + 8 + 16 * 8 + 16 * 4 == 216
    offs = {f[0]: getattr(_lib.ScaleRowsParams, f[0]).offset for f in fields}
    assert offs == {"struct_bytes": 0, "dtype": 4, "rows": 8, "segments": 12, "scale_rows": 16, "data": 24, "row_elems": 152}


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no host C compiler")
def test_block_size_equals_sizeof_from_the_header(tmp_path):
    from imagdressing_amd import _lib
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "imagdressing_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(imd_scale_rows_params), offsetof(imd_scale_rows_params, scale_rows),\n'
                   '                        offsetof(imd_scale_rows_params, data), offsetof(imd_scale_rows_params, row_elems)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _lib.ScaleRowsParams
    assert got == [ctypes.sizeof(P), P.scale_rows.offset, P.data.offset, P.row_elems.offset]


def launchable_block(segments=3):
    """a block that would launch: the fake addresses are never dereferenced on the host"""
    from imagdressing_amd import _lib
    p = _lib.ScaleRowsParams()
    p.dtype, p.rows, p.segments, p.scale_rows = 1, 4, segments, 0x300000
    for k in range(segments):
        p.data[k] = 0x100000 + 0x10000 * k
        p.row_elems[k] = 8 * (k + 1)
    return p


def test_foreign_struct_size_and_null_params_are_refused(lib):
    from imagdressing_amd import _lib
    size = ctypes.sizeof(_lib.ScaleRowsParams)
    for bad in (size - 8, size + 8, ctypes.sizeof(_lib.LoraRowsParams), 0):
        q = _lib.ScaleRowsParams()          # every field is 0: a library that read on would answer "unknown dtype" / "segments" instead
        q.dtype = 7
        q.struct_bytes = bad
        assert lib.imd_residual_scale_rows(ctypes.byref(q), None) != 0
        assert lib.imd_last_error().startswith(b"residual_scale_rows:") and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_residual_scale_rows(None, None) != 0 and b"residual_scale_rows: null params" in lib.imd_last_error()


def _set(p, over):
    for k, v in over.items():
        if isinstance(k, tuple):
            getattr(p, k[0])[k[1]] = v
        else:
            setattr(p, k, v)


REFUSALS = [({"segments": 0}, b"segments (0) outside 1..16"), ({"segments": 17}, b"segments (17) outside 1..16"), ({"segments": -1}, b"outside 1..16"),
            ({"rows": 0}, b"rows (0) must be at least 1"), ({"rows": -3}, b"rows (-3) must be at least 1"),
            ({("row_elems", 0): 0}, b"row_elems[0] (0) must be a positive multiple of 8"), ({("row_elems", 1): -8}, b"row_elems[1] (-8)"),
            ({("row_elems", 2): 12}, b"row_elems[2] (12) must be a positive multiple of 8"), ({("row_elems", 1): 4}, b"row_elems[1] (4)"),
            ({("data", 0): None}, b"null data[0]"), ({("data", 2): None}, b"null data[2]"),
            ({("data", 1): 0x110008}, b"data[1] must be 16-byte aligned"), ({("data", 0): 0x100002}, b"data[0] must be 16-byte aligned"),
            ({("data", 2): 0x120004}, b"data[2] must be 16-byte aligned"),
            ({"scale_rows": None}, b"null scale_rows"), ({"scale_rows": 0x300002}, b"scale_rows must be 4-byte aligned"),
            ({"scale_rows": 0x300001}, b"scale_rows must be 4-byte aligned"),
            ({"dtype": 2}, b"unknown dtype 2"), ({"dtype": -1}, b"unknown dtype -1"),
            ({"rows": 1 << 30, ("row_elems", 0): 8 * 4096}, b"too large")]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_precede_the_launch(lib, case):
    """an error code and a message by name, no launch (there is no GPU here, and the fake addresses are never touched)"""
    over, word = REFUSALS[case]
    p = launchable_block()
    _set(p, over)
    assert lib.imd_residual_scale_rows(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"residual_scale_rows:") and word in err and b"launch failed" not in err, err


def test_entries_past_segments_are_not_checked(lib):
    """segments = 3: data[3..15] are NULL and row_elems[3..15] are 0 in a launchable block; a bad entry among the first three is named"""
    p = launchable_block(16)
    p.data[15] = 0x8
    assert lib.imd_residual_scale_rows(ctypes.byref(p), None) != 0 and b"data[15] must be 16-byte aligned" in lib.imd_last_error()
    q = launchable_block(3)
    q.segments = 4
    assert lib.imd_residual_scale_rows(ctypes.byref(q), None) != 0 and b"row_elems[3] (0)" in lib.imd_last_error()


def test_the_wrapper_checks_its_operands_and_has_no_cpu_path():
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    h = torch.float16
    ok = [torch.zeros(4, 2, 2, 8, dtype=h), torch.zeros(4, 16, dtype=h)]
    s = torch.ones(4)
    with pytest.raises(ImdError, match="list of 1 to 16 tensors"):
        ops.residual_scale_rows([], s)
    with pytest.raises(ImdError, match="list of 1 to 16 tensors, got 17"):
        ops.residual_scale_rows([ok[1]] * 17, s)
    with pytest.raises(ImdError, match="list of 1 to 16 tensors"):
        ops.residual_scale_rows(ok[0], s)
    with pytest.raises(ImdError, match="must be a torch.Tensor"):
        ops.residual_scale_rows([ok[0], None], s)
    with pytest.raises(ImdError, match=r"differ in shape\[0\]"):
        ops.residual_scale_rows([ok[0], torch.zeros(3, 16, dtype=h)], s)
    with pytest.raises(ImdError, match="differ in dtype"):
        ops.residual_scale_rows([ok[0], torch.zeros(4, 16, dtype=torch.bfloat16)], s)
    with pytest.raises(ImdError, match="scale_rows must be a 1-d fp32 device tensor of 4 values"):
        ops.residual_scale_rows(ok, torch.ones(8))
    with pytest.raises(ImdError, match="scale_rows must be a 1-d fp32 device tensor of 4 values"):
        ops.residual_scale_rows(ok, torch.ones(4, 1))
    with pytest.raises(ImdError, match="scale_rows must be"):
        ops.residual_scale_rows(ok, [1.0] * 4)
    with pytest.raises(ImdError, match="bfloat16 or float16"):
        ops.residual_scale_rows([torch.zeros(4, 16)], s)
    with pytest.raises(ImdError, match=r"tensor 1 \(4, 12\): a row must hold a positive multiple of 8"):
        ops.residual_scale_rows([ok[1], torch.zeros(4, 12, dtype=h)], s)
    with pytest.raises(ImdError, match="tensor 0 must be contiguous"):
        ops.residual_scale_rows([torch.zeros(4, 32, dtype=h)[:, :16]], s)
    before = ops.SCALE_ROWS_COUNTER["launches"]
    with pytest.raises(ImdError, match="no CPU path"):          # well-formed operands on the host: refused, nothing computed
        ops.residual_scale_rows(ok, s)
    assert ops.SCALE_ROWS_COUNTER["launches"] == before and not ok[0].any()
