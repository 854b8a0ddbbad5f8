"""C ABI of the device noise source (imd_noise_rows / imd_noise_params) without a GPU: declared, bound, exported, listed in build.sh, the
ABI version unchanged (additive), the ctypes mirror equal to the header name for name with the sizes and offsets a C compiler gives it,
no step parameter block grown, and every refusal of the launcher, by message -- all precede the launch."""
import ctypes
import os
import re

import pytest

from tests.test_abi import HEADER, declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "imd_noise_rows"


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def launchable_block():
    """aligned fake addresses, never dereferenced on the host"""
    from imagdressing_amd import _lib
    p = _lib.NoiseParams()
    p.out, p.key_rows, p.rows, p.HW, p.kind = 0x1000, 0x2000, 1, 1, 0
    return p


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    assert NAME in declared_functions()
    assert NAME in _lib.SYMBOLS and hasattr(lib, NAME)
    assert sorted(_lib.SYMBOLS) == declared_functions()
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert callable(ops.noise_rows) and callable(ops.noise_key_row)
    assert "noise.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read().split()
    assert os.path.isfile(os.path.join(ROOT, "imagdressing_amd", "csrc", "noise.hip"))


def test_header_constants():
    from imagdressing_amd import _lib, ops
    text = open(HEADER).read()
    defs = dict(re.findall(r"#define (IMD_NOISE_[A-Z_]+)\s+(\d+)", text))
    assert defs == {"IMD_NOISE_ROW_WORDS": "8", "IMD_NOISE_NORMAL": "0", "IMD_NOISE_BITS": "1"}
    assert _lib.NOISE_ROW_WORDS == ops.NOISE_ROW_WORDS == 8 and _lib.NOISE_KINDS == {"normal": 0, "bits": 1}


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.NoiseParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_noise_params")
    assert [f[0] for f in fields] == ["struct_bytes", "out", "key_rows", "rows", "HW", "kind"]
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert kinds["out"] is ctypes.c_void_p and kinds["key_rows"] is ctypes.c_void_p
    assert kinds["rows"] is ctypes.c_int and kinds["HW"] is ctypes.c_int and kinds["kind"] is ctypes.c_int
    # LP64: uint32 + 4 pad, two pointers, three ints + 4 tail pad
    assert ctypes.sizeof(_lib.NoiseParams) == 40
    offs = {f[0]: getattr(_lib.NoiseParams, f[0]).offset for f in fields}
    assert offs == {"struct_bytes": 0, "out": 8, "key_rows": 16, "rows": 24, "HW": 28, "kind": 32}


def test_no_step_block_grew():
    """the noise is a launch of its own in front of the step: the parameter blocks of the step entry points are what they were"""
    from imagdressing_amd import _lib
    for cname, py, size, last in (("imd_sampler_params", _lib.SamplerParams, 168, "coefs"), ("imd_unipc_params", _lib.UnipcParams, 184, "coefs"),
                                  ("imd_ddim_params", _lib.DdimParams, 128, "sigma")):
        names = [f[0] for f in py._fields_]
        assert names == header_struct_fields(cname)
        assert names[-1] == last and not any("seed" in n or "key" in n for n in names)
        assert ctypes.sizeof(py) == size, (cname, ctypes.sizeof(py))


def test_foreign_struct_size_and_null_params_are_refused(lib):
    from imagdressing_amd import _lib
    p = _lib.NoiseParams()
    assert p.struct_bytes == ctypes.sizeof(_lib.NoiseParams)
    for bad in (p.struct_bytes - 8, p.struct_bytes + 8, ctypes.sizeof(_lib.SamplerParams), 0):
        q = _lib.NoiseParams()
        q.struct_bytes = bad            # out is NULL: a library that read on would answer "null out" instead
        assert lib.imd_noise_rows(ctypes.byref(q), None) != 0
        assert lib.imd_last_error().startswith(b"noise_rows:") and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_noise_rows(None, None) != 0 and b"noise_rows: null params" in lib.imd_last_error()
    assert lib.imd_noise_rows(ctypes.byref(p), None) != 0 and b"noise_rows: null out" in lib.imd_last_error()


REFUSALS = [(dict(out=None), b"null out"), (dict(key_rows=None), b"null key_rows"),
            (dict(out=0x1008), b"out must be 16-byte aligned"), (dict(out=0x1004), b"16-byte"), (dict(out=0x1001), b"16-byte"),
            (dict(key_rows=0x2008), b"key_rows must be 16-byte aligned"), (dict(key_rows=0x2004), b"key_rows must be 16-byte aligned"),
            (dict(rows=0), b"empty output"), (dict(rows=-1), b"empty output"), (dict(HW=0), b"empty output"), (dict(HW=-5), b"empty output"),
            (dict(rows=65536), b"at most 65535"),
            (dict(kind=2), b"unknown kind 2"), (dict(kind=-1), b"unknown kind -1")]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_launcher_refusals_precede_the_launch(lib, case):
    over, word = REFUSALS[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_noise_rows(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"noise_rows:") and word in err and b"launch failed" not in err, err


def test_the_wrapper_has_no_cpu_path_and_checks_its_operands():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    keys = ops.noise_key_rows([ops.noise_key_row(1, 0, 0)])
    assert keys.dtype == torch.int32 and tuple(keys.shape) == (1, 8)
    with pytest.raises(ImdError):
        ops.noise_rows(torch.zeros(1, 4, 4), keys)
    with pytest.raises(ImdError, match="unknown kind"):
        ops.noise_rows(torch.zeros(1, 4, 4), keys, kind="uniform")
    with pytest.raises(ImdError, match=r"\[rows, HW, 4\]"):
        ops.noise_rows(torch.zeros(1, 4, 3), keys)
