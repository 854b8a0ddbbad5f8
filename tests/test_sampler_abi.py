"""C ABI of the fused sampler step (imd_sampler_step / imd_sampler_params) without a GPU: declared, bound, exported, the ctypes
mirror equal to the header name for name, a foreign struct size refused before any field is read, and the launcher's refusals
(which all precede the launch)."""
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


def test_sampler_step_declared_bound_exported(lib):
    from imagdressing_amd import _lib
    assert "imd_sampler_step" in declared_functions()
    assert "imd_sampler_step" in _lib.SYMBOLS and hasattr(lib, "imd_sampler_step")
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert "imd_sampler_step" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.SamplerParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_sampler_params")
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert kinds["z_h"] is ctypes.c_float * 4 and kinds["store"] is ctypes.c_int and kinds["K"] is ctypes.c_int
    for ptr in ("z", "eps", "x_next", "hist", "guidance_rows", "noise", "mask", "z_img", "blend_noise", "coefs"):
        assert kinds[ptr] is ctypes.c_void_p, ptr
    from imagdressing_amd import ops
    text = open(os.path.join(ROOT, "include", "imagdressing_hip.h")).read()
    assert f"#define IMD_SAMPLER_COEFS {ops.SAMPLER_COEFS}" in text and f"#define IMD_SAMPLER_MAX_HISTORY {ops.SAMPLER_MAX_HISTORY}" in text


def test_foreign_struct_size_is_refused(lib):
    from imagdressing_amd import _lib
    p = _lib.SamplerParams()
    assert p.struct_bytes == ctypes.sizeof(_lib.SamplerParams)
    for bad in (ctypes.sizeof(_lib.SamplerParams) - 8, ctypes.sizeof(_lib.SamplerParams) + 8, 0):
        p.struct_bytes = bad            # every pointer is NULL: a library that read on would answer "null pointer" instead
        assert lib.imd_sampler_step(ctypes.byref(p), None) != 0
        assert b"sampler_step" in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_sampler_step(None, None) != 0 and b"null params" in lib.imd_last_error()
    q = _lib.SamplerParams()
    assert lib.imd_sampler_step(ctypes.byref(q), None) != 0 and b"null pointer" in lib.imd_last_error()


def refusal_cases():
    """(field overrides, word of the error) on top of a block that would otherwise launch; addresses are never dereferenced on the host"""
    return [(dict(K=5), b"K (5)"), (dict(K=-1, hist=None), b"K (-1)"), (dict(K=2, hist=None), b"without a history buffer"),
            (dict(K=2, store=2), b"store slot 2"), (dict(K=0, hist=None, store=0), b"store slot 0"), (dict(store=-2), b"store slot -2"),
            (dict(mask=0x4000), b"inpaint mask"), (dict(mask=0x4000, z_img=0x5000), b"inpaint mask"),
            (dict(mask=0x4000, blend_noise=0x5000), b"inpaint mask"),
            (dict(z=0x1008), b"16-byte"), (dict(eps=0x2004), b"16-byte"), (dict(x_next=0x3002), b"16-byte"), (dict(hist=0x6008), b"16-byte"),
            (dict(noise=0x7004), b"16-byte"), (dict(mask=0x4000, z_img=0x5008, blend_noise=0x8000), b"16-byte"),
            (dict(mask=0x4002, z_img=0x5000, blend_noise=0x8000), b"4-byte"), (dict(guidance_rows=0x9001), b"4-byte"),
            (dict(coefs=0xa002), b"4-byte"), (dict(B=0), b"empty latent"), (dict(dtype=7), b"unknown dtype")]


def launchable_block():
    from imagdressing_amd import _lib
    p = _lib.SamplerParams()
    p.z, p.eps, p.x_next, p.hist = 0x1000, 0x2000, 0x3000, 0x6000
    p.B, p.HW, p.K, p.dtype, p.store = 1, 1, 2, 1, -1
    return p


@pytest.mark.parametrize("case", range(len(refusal_cases())))
def test_launcher_refusals_precede_the_launch(lib, case):
    """K outside 0..4, store outside -1..K-1, a mask without its two companions, misaligned pointers: an error code and a message,
    no launch (there is no GPU here, and the fake addresses are never touched)"""
    over, word = refusal_cases()[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_sampler_step(ctypes.byref(p), None) != 0
    assert word in lib.imd_last_error() and b"launch failed" not in lib.imd_last_error(), lib.imd_last_error()


def test_sampler_step_has_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    with pytest.raises(ImdError):
        ops.sampler_step(torch.zeros(2, 4, 4), torch.zeros(4, 4, 4), None, guidance=7.5, coefs=ops.sampler_coefs())
