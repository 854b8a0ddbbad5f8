"""C ABI of the residual mix (imd_residual_mix_rows / imd_mix_rows_params) without a GPU: declared, bound, exported, listed in build.sh,
the ABI version unchanged (a new symbol only), the ctypes mirror equal to the header name for name and byte for byte, every refusal by
name before any launch, and the argument checks of ``ops.residual_mix_rows``."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.test_abi import HEADER, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "imd_residual_mix_rows"


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def header_fields(name):
    """the field names of a struct in the header, arrays of any rank included"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        for part in decl.split(","):
            part = re.sub(r"(\[\d+\])+\s*$", "", part.strip())
            if part:
                out.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)$", part)[0])
    return out


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    assert NAME in declared_functions()
    assert NAME in _lib.SYMBOLS and hasattr(lib, NAME)
    assert sorted(_lib.SYMBOLS) == declared_functions()
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # a new symbol only: the version stays
    assert callable(ops.residual_mix_rows)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "residual_mix_rows.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read().split()
    assert os.path.isfile(os.path.join(ROOT, "imagdressing_amd", "csrc", "residual_mix_rows.hip"))
    assert "imd_launch_residual_mix_rows" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "imd_kernels.h")).read()


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.MixRowsParams._fields_
    assert [f[0] for f in fields] == header_fields("imd_mix_rows_params")
    assert [f[0] for f in fields] == ["struct_bytes", "dtype", "rows", "segments", "sources", "scales", "src", "dst", "row_elems"]
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert all(kinds[k] is ctypes.c_int for k in ("dtype", "rows", "segments", "sources"))
    assert kinds["scales"] is ctypes.c_void_p
    assert kinds["src"]._length_ == _lib.MIX_ROWS_MAX_SOURCES == 4 and kinds["src"]._type_._length_ == _lib.MIX_ROWS_MAX_SEGMENTS == 16
    assert kinds["src"]._type_._type_ is ctypes.c_void_p
    assert kinds["dst"]._length_ == kinds["row_elems"]._length_ == 16
    assert kinds["dst"]._type_ is ctypes.c_void_p and kinds["row_elems"]._type_ is ctypes.c_int
    text = open(HEADER).read()
    assert "#define IMD_MIX_ROWS_MAX_SOURCES 4" in text and "#define IMD_MIX_ROWS_MAX_SEGMENTS 16" in text
    assert "const void* src[4][16]" in text
    # LP64: uint32 + 4 ints (20 bytes, padded to 24), a pointer, 64 + 16 pointers, 16 ints
    assert ctypes.sizeof(_lib.MixRowsParams) == 24 + 8 + 64 * 8 + 16 * 8 + 16 * 4 == 736
    offs = {f[0]: getattr(_lib.MixRowsParams, f[0]).offset for f in fields}
    assert offs == {"struct_bytes": 0, "dtype": 4, "rows": 8, "segments": 12, "sources": 16, "scales": 24, "src": 32, "dst": 544,
                    "row_elems": 672}


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no host C compiler")
def test_block_size_equals_sizeof_from_the_header(tmp_path):
    from imagdressing_amd import _lib
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "imagdressing_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(imd_mix_rows_params), offsetof(imd_mix_rows_params, scales),\n'
                   '                        offsetof(imd_mix_rows_params, src), offsetof(imd_mix_rows_params, dst),\n'
                   '                        offsetof(imd_mix_rows_params, row_elems), sizeof(((imd_mix_rows_params*)0)->src[0])); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _lib.MixRowsParams
    assert got == [ctypes.sizeof(P), P.scales.offset, P.src.offset, P.dst.offset, P.row_elems.offset, 16 * 8]


SRC0, DST0, STEP = 0x1000000, 0x9000000, 0x100000


def launchable_block(segments=3, sources=2):
    """a block that would launch: the fake addresses are never dereferenced on the host"""
    from imagdressing_amd import _lib
    p = _lib.MixRowsParams()
    p.dtype, p.rows, p.segments, p.sources, p.scales = 1, 4, segments, sources, 0x300000
    for j in range(segments):
        for k in range(sources):
            p.src[k][j] = SRC0 + STEP * (16 * k + j)
        p.dst[j] = DST0 + STEP * j
        p.row_elems[j] = 8 * (j + 1)
    return p


def test_foreign_struct_size_and_null_params_are_refused(lib):
    from imagdressing_amd import _lib
    size = ctypes.sizeof(_lib.MixRowsParams)
    for bad in (size - 8, size + 8, ctypes.sizeof(_lib.ScaleRowsParams), 0):
        q = _lib.MixRowsParams()          # every field is 0: a library that read on would answer "unknown dtype" / "sources" instead
        q.dtype = 7
        q.struct_bytes = bad
        assert lib.imd_residual_mix_rows(ctypes.byref(q), None) != 0
        assert lib.imd_last_error().startswith(b"residual_mix_rows:") and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_residual_mix_rows(None, None) != 0 and b"residual_mix_rows: null params" in lib.imd_last_error()


def _set(p, over):
    for k, v in over.items():
        if isinstance(k, tuple) and len(k) == 3:
            getattr(p, k[0])[k[1]][k[2]] = v
        elif isinstance(k, tuple):
            getattr(p, k[0])[k[1]] = v
        else:
            setattr(p, k, v)


SEG0 = 4 * 8 * 2           # bytes of segment 0 of the launchable block: 4 rows of 8 elements
REFUSALS = [({"sources": 0}, b"sources (0) outside 1..4"), ({"sources": 5}, b"sources (5) outside 1..4"), ({"sources": -1}, b"outside 1..4"),
            ({"segments": 0}, b"segments (0) outside 1..16"), ({"segments": 17}, b"segments (17) outside 1..16"),
            ({"rows": 0}, b"rows (0) must be at least 1"), ({"rows": -3}, b"rows (-3) must be at least 1"),
            ({"scales": None}, b"null scales"), ({"scales": 0x300002}, b"scales must be 4-byte aligned"),
            ({"scales": 0x300001}, b"scales must be 4-byte aligned"),
            ({("row_elems", 0): 0}, b"row_elems[0] (0) must be a positive multiple of 8"), ({("row_elems", 1): -8}, b"row_elems[1] (-8)"),
            ({("row_elems", 2): 12}, b"row_elems[2] (12) must be a positive multiple of 8"),
            ({("dst", 0): None}, b"null dst[0]"), ({("dst", 2): 0x9200008}, b"dst[2] must be 16-byte aligned"),
            ({("src", 0, 0): None}, b"null src[0][0]"), ({("src", 1, 2): None}, b"null src[1][2]"),
            ({("src", 1, 1): SRC0 + 4}, b"src[1][1] must be 16-byte aligned"), ({("src", 0, 2): SRC0 + 2}, b"src[0][2] must be 16-byte aligned"),
            ({"dtype": 2}, b"unknown dtype 2"), ({"dtype": -1}, b"unknown dtype -1"),
            ({"rows": 1 << 30, ("row_elems", 0): 8 * 4096}, b"too large"),
            # overlap: dst[1] inside src[0][1], behind it by one vector, on another segment of a source, on another dst segment
            ({("dst", 1): SRC0 + STEP + 16}, b"dst[1] overlaps src[0][1]"),
            ({("dst", 1): SRC0 + STEP - 16}, b"dst[1] overlaps src[0][1]"),
            ({("dst", 1): SRC0 + STEP * 16 + SEG0 - 16}, b"dst[1] overlaps src[1][0]"),
            ({("dst", 0): SRC0 + STEP}, b"dst[0] overlaps src[0][1]"),
            ({("dst", 2): DST0 + STEP + 16}, b"overlaps dst[")]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_precede_the_launch(lib, case):
    """an error code and a message by name, no launch (there is no GPU here, and the fake addresses are never touched)"""
    over, word = REFUSALS[case]
    p = launchable_block()
    _set(p, over)
    assert lib.imd_residual_mix_rows(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"residual_mix_rows:") and word in err and b"launch failed" not in err, err


def test_entries_past_sources_and_segments_are_not_checked(lib):
    p = launchable_block(3, 2)          # src[2..3][*], src[*][3..15], dst[3..15] are NULL, row_elems[3..15] are 0
    p.sources = 3
    assert lib.imd_residual_mix_rows(ctypes.byref(p), None) != 0 and b"null src[2][0]" in lib.imd_last_error()
    q = launchable_block(3, 2)
    q.segments = 4
    assert lib.imd_residual_mix_rows(ctypes.byref(q), None) != 0 and b"row_elems[3] (0)" in lib.imd_last_error()


def test_the_wrapper_checks_its_operands_and_has_no_cpu_path():
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    h = torch.float16
    a = [torch.zeros(4, 2, 2, 8, dtype=h), torch.zeros(4, 16, dtype=h)]
    b = [torch.ones(4, 2, 2, 8, dtype=h), torch.ones(4, 16, dtype=h)]
    s = torch.ones(2, 4)
    with pytest.raises(ImdError, match="list of 1 to 4 sources, got 0"):
        ops.residual_mix_rows([], s)
    with pytest.raises(ImdError, match="list of 1 to 4 sources, got 5"):
        ops.residual_mix_rows([a] * 5, torch.ones(5, 4))
    with pytest.raises(ImdError, match="source 1: expected a list of 1 to 16 tensors, got 17"):
        ops.residual_mix_rows([a, [a[1]] * 17], s)
    with pytest.raises(ImdError, match="source 0: expected a list of 1 to 16 tensors"):
        ops.residual_mix_rows([a[0], b[0]], s)
    with pytest.raises(ImdError, match="source 1: every segment must be a torch.Tensor"):
        ops.residual_mix_rows([a, [b[0], None]], s)
    with pytest.raises(ImdError, match="source 1 has 1 segments, source 0 has 2"):
        ops.residual_mix_rows([a, b[:1]], s)
    with pytest.raises(ImdError, match=r"source 1, tensor 1: shape \(3, 16\) differs from source 0's \(4, 16\)"):
        ops.residual_mix_rows([a, [b[0], torch.zeros(3, 16, dtype=h)]], s)
    with pytest.raises(ImdError, match="source 1, tensor 1: the tensors differ in dtype"):
        ops.residual_mix_rows([a, [b[0], torch.zeros(4, 16, dtype=torch.bfloat16)]], s)
    with pytest.raises(ImdError, match=r"scales must be an fp32 device tensor \[2, 4\]"):
        ops.residual_mix_rows([a, b], torch.ones(4, 2))
    with pytest.raises(ImdError, match=r"scales must be an fp32 device tensor \[2, 4\]"):
        ops.residual_mix_rows([a, b], torch.ones(8))
    with pytest.raises(ImdError, match="scales must be"):
        ops.residual_mix_rows([a, b], [[1.0] * 4] * 2)
    with pytest.raises(ImdError, match="out has 1 segments, source 0 has 2"):
        ops.residual_mix_rows([a, b], s, out=a[:1])
    with pytest.raises(ImdError, match="out must be None or a list of tensors"):
        ops.residual_mix_rows([a, b], s, out=a[0])
    with pytest.raises(ImdError, match="bfloat16 or float16"):
        ops.residual_mix_rows([[torch.zeros(4, 16)]], torch.ones(1, 4))
    with pytest.raises(ImdError, match=r"tensor 0 \(4, 12\): a row must hold a positive multiple of 8"):
        ops.residual_mix_rows([[torch.zeros(4, 12, dtype=h)]], torch.ones(1, 4))
    with pytest.raises(ImdError, match="source 0, tensor 0 must be contiguous"):
        ops.residual_mix_rows([[torch.zeros(4, 32, dtype=h)[:, :16]]], torch.ones(1, 4))
    before = ops.MIX_ROWS_COUNTER["launches"]
    with pytest.raises(ImdError, match="no CPU path"):          # well-formed operands on the host: refused, nothing computed
        ops.residual_mix_rows([a, b], s, out=a)
    assert ops.MIX_ROWS_COUNTER["launches"] == before and not a[0].any()
