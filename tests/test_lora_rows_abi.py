"""C ABI of the per-row LoRA expansion (imd_lora_expand_rows / imd_lora_rows_params) without a GPU: declared, bound, exported, the
ctypes mirror equal to the header name for name, a foreign struct size refused before any field is read, and every refusal of the
launcher (which all precede the launch)."""
import ctypes
import os

import pytest

from tests.test_abi import declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    assert "imd_lora_expand_rows" in declared_functions()
    assert "imd_lora_expand_rows" in _lib.SYMBOLS and hasattr(lib, "imd_lora_expand_rows")
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert callable(ops.lora_expand_rows)
    assert "imd_lora_expand_rows" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lora_rows.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read()


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.LoraRowsParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_lora_rows_params")
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    for ptr in ("x", "down", "row_scale", "out"):
        assert kinds[ptr] is ctypes.c_void_p, ptr
    for i in ("M", "C", "T", "E", "rows_per_entry", "x_ld", "out_ld", "dtype"):
        assert kinds[i] is ctypes.c_int, i
    # uint32 + padding, 4 pointers, 8 ints
    assert ctypes.sizeof(_lib.LoraRowsParams) == 8 + 4 * 8 + 8 * 4


def test_foreign_struct_size_is_refused(lib):
    from imagdressing_amd import _lib
    p = _lib.LoraRowsParams()
    size = ctypes.sizeof(_lib.LoraRowsParams)
    assert p.struct_bytes == size
    for bad in (size - 8, size + 8, 0):
        p.struct_bytes = bad            # every pointer is NULL: a library that read on would answer "null pointer" instead
        assert lib.imd_lora_expand_rows(ctypes.byref(p), None) != 0
        assert b"lora_expand_rows" in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_lora_expand_rows(None, None) != 0 and b"null params" in lib.imd_last_error()
    q = _lib.LoraRowsParams()
    assert lib.imd_lora_expand_rows(ctypes.byref(q), None) != 0 and b"null pointer" in lib.imd_last_error()


def launchable_block():
    """a block that would launch: addresses are never dereferenced on the host"""
    from imagdressing_amd import _lib
    p = _lib.LoraRowsParams()
    p.x, p.down, p.row_scale, p.out = 0x100000, 0x200000, 0x300000, 0x400000
    p.M, p.C, p.T, p.E, p.rows_per_entry = 64, 320, 128, 4, 16
    p.x_ld, p.out_ld, p.dtype = 320, 448, 1
    return p


def refusal_cases():
    return [(dict(C=328), b"multiples of 16"), (dict(C=72, x_ld=72), b"multiples of 16"), (dict(T=120), b"multiples of 16"), (dict(T=8), b"multiples of 16"),
            (dict(C=1296, x_ld=1296, out_ld=1424), b"outside 64..1280"), (dict(C=48, x_ld=48), b"outside 64..1280"), (dict(C=0), b"outside 64..1280"),
            (dict(T=400, out_ld=720), b"outside 16..384"), (dict(T=0), b"outside 16..384"),
            (dict(M=65), b"rows_per_entry"), (dict(E=3), b"rows_per_entry"), (dict(rows_per_entry=0), b"rows_per_entry"), (dict(M=0, E=0), b"rows_per_entry"),
            (dict(E=-4, rows_per_entry=-16), b"rows_per_entry"),
            (dict(x_ld=312), b"x_ld (312) < C"), (dict(out_ld=440), b"out_ld (440) < C + T"),
            (dict(x_ld=324), b"multiples of 8"), (dict(out_ld=452), b"multiples of 8"),
            (dict(x=0x100008), b"16-byte"), (dict(down=0x200004), b"16-byte"), (dict(out=0x400002), b"16-byte"), (dict(row_scale=0x300002), b"4-byte"),
            (dict(out=0x100000), b"overlaps"), (dict(out=0x100000 + 63 * 640 + 320), b"overlaps"), (dict(x=0x400000 + 63 * 896 + 640), b"overlaps"),
            (dict(dtype=7), b"unknown dtype"),
            (dict(M=1 << 22, E=1 << 18, x_ld=1024, out_ld=1024), b"too large")]


@pytest.mark.parametrize("case", range(len(refusal_cases())))
def test_launcher_refusals_precede_the_launch(lib, case):
    """an error code and a message, no launch (there is no GPU here, and the fake addresses are never touched)"""
    over, word = refusal_cases()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_lora_expand_rows(ctypes.byref(p), None) != 0
    assert word in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error(), lib.imd_last_error()


def test_lora_expand_rows_has_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    with pytest.raises(ImdError):
        ops.lora_expand_rows(torch.zeros(64, 320, dtype=torch.float16), torch.zeros(16, 320, dtype=torch.float16), torch.ones(4), 16)
