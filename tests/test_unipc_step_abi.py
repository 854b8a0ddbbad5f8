"""C ABI of the fused UniPC step (imd_unipc_step, imd_unipc_step_rows, imd_unipc_step_rows_at / imd_unipc_params) without a GPU:
declared, bound, exported, the ABI version unchanged (additive), the ctypes mirror equal to the header name for name, a foreign
struct size refused before any field is read, and every refusal of the three launchers, by message -- all precede the launch."""
import ctypes
import os

import pytest

from tests.test_abi import declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, MAP = 0xb000, 0xc000          # aligned fake addresses: never dereferenced on the host
NAMES = ("imd_unipc_step", "imd_unipc_step_rows", "imd_unipc_step_rows_at")


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def call(lib, form, p, rows=ROWS, row_slot=MAP, slots=4):
    ref = None if p is None else ctypes.byref(p)
    if form == "unipc_step":
        return lib.imd_unipc_step(ref, None)
    if form == "unipc_step_rows":
        return lib.imd_unipc_step_rows(ref, rows, None)
    return lib.imd_unipc_step_rows_at(ref, rows, row_slot, slots, None)


FORMS = ("unipc_step", "unipc_step_rows", "unipc_step_rows_at")


def launchable_block():
    from imagdressing_amd import _lib
    p = _lib.UnipcParams()
    p.z, p.eps, p.x_next, p.hist = 0x1000, 0x2000, 0x3000, 0x6000
    p.B, p.HW, p.K, p.dtype, p.store_m, p.store_s = 1, 1, 3, 1, -1, -1
    return p


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in declared_functions()
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in text
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert all(callable(getattr(ops, n)) for n in ("unipc_coefs", "unipc_step", "unipc_step_rows", "unipc_step_rows_at"))
    assert "unipc_step.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read()


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib, ops
    fields = _lib.UnipcParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_unipc_params")
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert kinds["s_h"] is ctypes.c_float * 4 and kinds["z_h"] is ctypes.c_float * 4
    assert kinds["store_m"] is ctypes.c_int and kinds["store_s"] is ctypes.c_int and kinds["K"] is ctypes.c_int
    for ptr in ("z", "eps", "x_next", "hist", "guidance_rows", "mask", "z_img", "blend_noise", "coefs"):
        assert kinds[ptr] is ctypes.c_void_p, ptr
    text = open(os.path.join(ROOT, "include", "imagdressing_hip.h")).read()
    assert f"#define IMD_UNIPC_COEFS {ops.UNIPC_COEFS}" in text and f"#define IMD_UNIPC_ROW_FLOATS {ops.UNIPC_ROW_FLOATS}" in text
    assert ops.UNIPC_ROW_FLOATS % 4 == 0 and ops.UNIPC_ROW_FLOATS > ops.UNIPC_COEFS          # 16-byte rows with room for `active`
    # imd_sampler_params did not grow
    assert [f[0] for f in _lib.SamplerParams._fields_] == header_struct_fields("imd_sampler_params")


@pytest.mark.parametrize("form", FORMS)
def test_foreign_struct_size_and_null_pointers_are_refused(lib, form):
    from imagdressing_amd import _lib
    p = _lib.UnipcParams()
    assert p.struct_bytes == ctypes.sizeof(_lib.UnipcParams)
    for bad in (ctypes.sizeof(_lib.UnipcParams) - 8, ctypes.sizeof(_lib.UnipcParams) + 8, ctypes.sizeof(_lib.SamplerParams), 0):
        p.struct_bytes = bad            # every pointer is NULL: a library that read on would answer "null pointer" instead
        assert call(lib, form, p) != 0
        assert lib.imd_last_error().startswith(form.encode() + b":") and b"parameter block is" in lib.imd_last_error()
    assert call(lib, form, None) != 0 and (form.encode() + b": null params") in lib.imd_last_error()
    q = _lib.UnipcParams()
    assert call(lib, form, q) != 0 and (form.encode() + b": null pointer") in lib.imd_last_error()


def shared_refusals():
    """(field overrides, word of the error) on top of a block that would otherwise launch -- what the three forms refuse alike"""
    return [(dict(K=5), b"K (5)"), (dict(K=-1, hist=None), b"K (-1)"), (dict(K=2, hist=None), b"without a history buffer"),
            (dict(mask=0x4000), b"inpaint mask"), (dict(mask=0x4000, z_img=0x5000), b"inpaint mask"),
            (dict(mask=0x4000, blend_noise=0x5000), b"inpaint mask"),
            (dict(z=0x1008), b"16-byte"), (dict(eps=0x2004), b"16-byte"), (dict(x_next=0x3002), b"16-byte"), (dict(hist=0x6008), b"16-byte"),
            (dict(mask=0x4000, z_img=0x5008, blend_noise=0x8000), b"16-byte"), (dict(mask=0x4000, z_img=0x5000, blend_noise=0x8004), b"16-byte"),
            (dict(mask=0x4002, z_img=0x5000, blend_noise=0x8000), b"4-byte"), (dict(guidance_rows=0x9001), b"4-byte"),
            (dict(B=0), b"empty latent"), (dict(dtype=7), b"unknown dtype")]


def scalar_refusals():
    """the host-coefficient form alone: the store slots are in -1..K-1 and distinct, the device block is 4-byte aligned"""
    return [(dict(store_m=3), b"store_m slot 3"), (dict(store_s=3), b"store_s slot 3"), (dict(store_m=-2), b"store_m slot -2"),
            (dict(store_s=-2), b"store_s slot -2"), (dict(K=0, hist=None, store_m=0), b"store_m slot 0"),
            (dict(store_m=1, store_s=1), b"the same slot 1"), (dict(store_m=0, store_s=0), b"the same slot 0"),
            (dict(coefs=0xa002), b"4-byte")]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", range(len(shared_refusals())))
def test_launcher_refusals_precede_the_launch(lib, form, case):
    over, word = shared_refusals()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert call(lib, form, p) != 0
    err = lib.imd_last_error()
    assert err.startswith(form.encode() + b":") and word in err and b"launch failed" not in err, err


@pytest.mark.parametrize("case", range(len(scalar_refusals())))
def test_store_slots_of_the_host_form(lib, case):
    over, word = scalar_refusals()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_unipc_step(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"unipc_step:") and word in err and b"launch failed" not in err, err


def test_rows_map_and_slots_are_checked(lib):
    p = launchable_block()
    for form in ("unipc_step_rows", "unipc_step_rows_at"):
        name = form.encode()
        assert call(lib, form, p, rows=None) != 0 and (name + b": null coef_rows") in lib.imd_last_error()
        for bad in (ROWS + 4, ROWS + 8, ROWS + 1):
            assert call(lib, form, p, rows=bad) != 0
            assert (name + b": coef_rows must be 16-byte aligned") in lib.imd_last_error()
    assert call(lib, "unipc_step_rows_at", p, row_slot=None) != 0 and b"unipc_step_rows_at: null row_slot" in lib.imd_last_error()
    assert call(lib, "unipc_step_rows_at", p, row_slot=MAP + 2) != 0
    assert b"unipc_step_rows_at: row_slot must be 4-byte aligned" in lib.imd_last_error()
    for slots in (0, -3):
        assert call(lib, "unipc_step_rows_at", p, slots=slots) != 0 and b"unipc_step_rows_at: slots" in lib.imd_last_error()
    p.B = 3
    assert call(lib, "unipc_step_rows_at", p, slots=2) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"unipc_step_rows_at: B (3") and b"exceeds slots (2)" in err and b"launch failed" not in err, err


def test_the_wrappers_have_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    z, eps = torch.zeros(2, 4, 4), torch.zeros(4, 4, 4)
    with pytest.raises(ImdError):
        ops.unipc_step(z, eps, None, guidance=7.5, coefs=ops.unipc_coefs())
    rows = torch.tensor([ops.unipc_coef_row(ops.unipc_coefs())] * 2)
    with pytest.raises(ImdError):
        ops.unipc_step_rows(z, eps, None, guidance=7.5, coef_rows=rows)
    with pytest.raises(ImdError):
        ops.unipc_step_rows_at(torch.zeros(3, 4, 4), eps, None, guidance=7.5, coef_rows=rows, row_slot=torch.tensor([1, 0], dtype=torch.int32))
