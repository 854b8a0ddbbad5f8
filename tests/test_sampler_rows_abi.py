"""C ABI of the per-row fused sampler step (imd_sampler_step_rows) without a GPU: declared, bound, exported, the ABI version
unchanged (additive), the row constants agree, and the launcher's refusals -- a foreign struct size, the coefficient rows missing or
misaligned, and every pointer / K / mask condition of imd_sampler_step -- all precede the launch."""
import ctypes
import os

import pytest

from tests.test_abi import declared_functions
from tests.test_sampler_abi import launchable_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 0xb000          # a 16-byte aligned fake address: never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_sampler_step_rows_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    assert "imd_sampler_step_rows" in declared_functions()
    assert "imd_sampler_step_rows" in _lib.SYMBOLS and hasattr(lib, "imd_sampler_step_rows")
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    text = open(os.path.join(ROOT, "include", "imagdressing_hip.h")).read()
    assert f"#define IMD_SAMPLER_ROW_FLOATS {ops.SAMPLER_ROW_FLOATS}" in text and ops.SAMPLER_ROW_FLOATS == 16
    assert "imd_sampler_step_rows" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_coef_row_layout():
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    c = ops.sampler_coefs(m_x=1.5, m_e=-2.0, z_x=0.5, z_m=0.25, z_h=(3.0, 4.0), z_n=5.0, b_img=6.0, b_noise=7.0, in_scale=8.0, store=1)
    row = ops.sampler_coef_row(c)
    assert len(row) == ops.SAMPLER_ROW_FLOATS and row[:13] == c and row[13:] == [1.0, 0.0, 0.0]
    assert ops.sampler_coef_row(c, active=False)[13:] == [0.0, 0.0, 0.0]
    with pytest.raises(ImdError):
        ops.sampler_coef_row(c[:12])


def test_foreign_struct_size_is_refused(lib):
    from imagdressing_amd import _lib
    p = _lib.SamplerParams()
    for bad in (ctypes.sizeof(_lib.SamplerParams) - 8, ctypes.sizeof(_lib.SamplerParams) + 8, 0):
        p.struct_bytes = bad            # every pointer is NULL: a library that read on would answer "null pointer" instead
        assert lib.imd_sampler_step_rows(ctypes.byref(p), ROWS, None) != 0
        assert b"sampler_step_rows" in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_sampler_step_rows(None, ROWS, None) != 0 and b"null params" in lib.imd_last_error()
    q = _lib.SamplerParams()
    assert lib.imd_sampler_step_rows(ctypes.byref(q), ROWS, None) != 0 and b"null pointer" in lib.imd_last_error()


def test_coef_rows_pointer_is_checked(lib):
    p = launchable_block()
    assert lib.imd_sampler_step_rows(ctypes.byref(p), None, None) != 0
    assert b"sampler_step_rows: null coef_rows" in lib.imd_last_error()
    for bad in (ROWS + 4, ROWS + 8, ROWS + 1):
        assert lib.imd_sampler_step_rows(ctypes.byref(p), bad, None) != 0
        assert b"coef_rows must be 16-byte aligned" in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error()


def refusal_cases():
    """the pointer, K and mask conditions of imd_sampler_step (tests/test_sampler_abi.py) -- without the host ``store`` checks (the
    store slot of every row lives in device memory; the kernel ignores one outside 0..K-1) and the ``coefs`` alignment (ignored)"""
    return [(dict(K=5), b"K (5)"), (dict(K=-1, hist=None), b"K (-1)"), (dict(K=2, hist=None), b"without a history buffer"),
            (dict(mask=0x4000), b"inpaint mask"), (dict(mask=0x4000, z_img=0x5000), b"inpaint mask"),
            (dict(mask=0x4000, blend_noise=0x5000), b"inpaint mask"),
            (dict(z=0x1008), b"16-byte"), (dict(eps=0x2004), b"16-byte"), (dict(x_next=0x3002), b"16-byte"), (dict(hist=0x6008), b"16-byte"),
            (dict(noise=0x7004), b"16-byte"), (dict(mask=0x4000, z_img=0x5008, blend_noise=0x8000), b"16-byte"),
            (dict(mask=0x4002, z_img=0x5000, blend_noise=0x8000), b"4-byte"), (dict(guidance_rows=0x9001), b"4-byte"),
            (dict(B=0), b"empty latent"), (dict(HW=0), b"empty latent"), (dict(dtype=7), b"unknown dtype")]


@pytest.mark.parametrize("case", range(len(refusal_cases())))
def test_launcher_refusals_precede_the_launch(lib, case):
    """an error code and a message in the launcher's own name, no launch (there is no GPU here, and the fake addresses are never touched)"""
    over, word = refusal_cases()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_sampler_step_rows(ctypes.byref(p), ROWS, None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"sampler_step_rows:") and word in err and b"launch failed" not in err, err


def test_sampler_step_rows_has_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    rows = torch.tensor([ops.sampler_coef_row(ops.sampler_coefs())] * 2)
    with pytest.raises(ImdError):
        ops.sampler_step_rows(torch.zeros(2, 4, 4), torch.zeros(4, 4, 4), None, guidance=7.5, coef_rows=rows)
