"""C ABI of the compacting session's two launches (imd_sampler_step_rows_at, imd_session_input_rows) without a GPU: declared, bound,
exported, the ABI version unchanged (additive), and the launchers' refusals -- a foreign struct size, the coefficient rows or the
row -> slot map missing or misaligned, more batch rows than slots, and every pointer / K / mask condition of imd_sampler_step_rows
-- all precede the launch."""
import ctypes
import os

import pytest

from tests.test_abi import declared_functions
from tests.test_sampler_abi import launchable_block
from tests.test_sampler_rows_abi import refusal_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, MAP, SCALES, Z, X = 0xb000, 0xc000, 0xd000, 0x1000, 0x3000          # aligned fake addresses: never dereferenced on the host
NAMES = ("imd_sampler_step_rows_at", "imd_session_input_rows")


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in declared_functions()
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in text
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert callable(ops.sampler_step_rows_at) and callable(ops.session_input_rows)


def test_foreign_struct_size_and_null_pointers_are_refused(lib):
    from imagdressing_amd import _lib
    p = _lib.SamplerParams()
    for bad in (ctypes.sizeof(_lib.SamplerParams) - 8, ctypes.sizeof(_lib.SamplerParams) + 8, 0):
        p.struct_bytes = bad
        assert lib.imd_sampler_step_rows_at(ctypes.byref(p), ROWS, MAP, 1, None) != 0
        assert b"sampler_step_rows_at" in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_sampler_step_rows_at(None, ROWS, MAP, 1, None) != 0 and b"sampler_step_rows_at: null params" in lib.imd_last_error()
    q = _lib.SamplerParams()
    assert lib.imd_sampler_step_rows_at(ctypes.byref(q), ROWS, MAP, 1, None) != 0 and b"sampler_step_rows_at: null pointer" in lib.imd_last_error()


def test_rows_map_and_slots_are_checked(lib):
    p = launchable_block()
    assert lib.imd_sampler_step_rows_at(ctypes.byref(p), None, MAP, 1, None) != 0
    assert b"sampler_step_rows_at: null coef_rows" in lib.imd_last_error()
    for bad in (ROWS + 4, ROWS + 8, ROWS + 1):
        assert lib.imd_sampler_step_rows_at(ctypes.byref(p), bad, MAP, 1, None) != 0
        assert b"sampler_step_rows_at: coef_rows must be 16-byte aligned" in lib.imd_last_error()
    assert lib.imd_sampler_step_rows_at(ctypes.byref(p), ROWS, None, 1, None) != 0
    assert b"sampler_step_rows_at: null row_slot" in lib.imd_last_error()
    assert lib.imd_sampler_step_rows_at(ctypes.byref(p), ROWS, MAP + 2, 1, None) != 0
    assert b"sampler_step_rows_at: row_slot must be 4-byte aligned" in lib.imd_last_error()
    for slots in (0, -3):
        assert lib.imd_sampler_step_rows_at(ctypes.byref(p), ROWS, MAP, slots, None) != 0
        assert b"sampler_step_rows_at: slots" in lib.imd_last_error()
    p.B = 3
    assert lib.imd_sampler_step_rows_at(ctypes.byref(p), ROWS, MAP, 2, None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"sampler_step_rows_at: B (3") and b"exceeds slots (2)" in err and b"launch failed" not in err, err


@pytest.mark.parametrize("case", range(len(refusal_cases())))
def test_launcher_refusals_precede_the_launch(lib, case):
    """the alignment and size refusals of imd_sampler_step_rows, in this launcher's name, no launch (there is no GPU here)"""
    over, word = refusal_cases()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_sampler_step_rows_at(ctypes.byref(p), ROWS, MAP, 4, None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"sampler_step_rows_at:") and word in err and b"launch failed" not in err, err


def test_session_input_rows_refusals(lib):
    ok = dict(z=Z, row_slot=MAP, in_scale_rows=SCALES, x_in=X, B=1, slots=2, HW=4, dtype=1)
    cases = [(dict(z=None), b"null pointer"), (dict(row_slot=None), b"null pointer"), (dict(in_scale_rows=None), b"null pointer"),
             (dict(x_in=None), b"null pointer"), (dict(B=0), b"empty input"), (dict(HW=0), b"empty input"), (dict(slots=0), b"slots (0)"),
             (dict(B=3), b"exceeds slots"), (dict(z=Z + 8), b"16-byte"), (dict(x_in=X + 4), b"16-byte"), (dict(row_slot=MAP + 2), b"4-byte"),
             (dict(in_scale_rows=SCALES + 1), b"4-byte"), (dict(dtype=7), b"unknown dtype")]
    for over, word in cases:
        a = dict(ok, **over)
        assert lib.imd_session_input_rows(a["z"], a["row_slot"], a["in_scale_rows"], a["x_in"], a["B"], a["slots"], a["HW"], a["dtype"], None) != 0
        err = lib.imd_last_error()
        assert err.startswith(b"session_input_rows:") and word in err and b"launch failed" not in err, (over, err)


def test_the_wrappers_have_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    rows = torch.tensor([ops.sampler_coef_row(ops.sampler_coefs())] * 2)
    rs = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(ImdError):
        ops.sampler_step_rows_at(torch.zeros(3, 4, 4), torch.zeros(4, 4, 4), None, guidance=7.5, coef_rows=rows, row_slot=rs)
    with pytest.raises(ImdError):
        ops.session_input_rows(torch.zeros(3, 4, 4), rs, torch.ones(2), torch.zeros(4, 4, 8, dtype=torch.float16))
