"""C ABI of the CFG rescale (imd_guidance_rescale / imd_guidance_rescale_params) without a GPU: declared, bound, exported, the ABI
version unchanged (additive), the ctypes mirror equal to the header name for name, no step parameter block grown, a foreign struct
size refused before any field is read, and every refusal of the launcher, by message -- all precede the launch."""
import ctypes
import os

import pytest

from tests.test_abi import declared_functions, header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "imd_guidance_rescale"


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
    p = _lib.GuidanceRescaleParams()
    p.eps, p.B, p.HW, p.guidance, p.rescale = 0x1000, 1, 1, 7.5, 0.7
    return p


def test_declared_bound_exported(lib):
    from imagdressing_amd import _lib, ops
    assert NAME in declared_functions()
    assert NAME in _lib.SYMBOLS and hasattr(lib, NAME)
    assert sorted(_lib.SYMBOLS) == declared_functions()
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.imd_abi_version() == _lib.ABI_VERSION == 9              # additive change: the version stays
    assert callable(ops.guidance_rescale)
    assert "guidance_rescale.hip" in open(os.path.join(ROOT, "imagdressing_amd", "csrc", "build.sh")).read()


def test_struct_layout_matches_header():
    from imagdressing_amd import _lib
    fields = _lib.GuidanceRescaleParams._fields_
    assert [f[0] for f in fields] == header_struct_fields("imd_guidance_rescale_params")
    assert [f[0] for f in fields] == ["struct_bytes", "eps", "B", "HW", "guidance", "guidance_rows", "rescale", "rescale_rows"]
    assert fields[0] == ("struct_bytes", ctypes.c_uint32)
    kinds = dict((f[0], f[1]) for f in fields)
    assert kinds["B"] is ctypes.c_int and kinds["HW"] is ctypes.c_int
    assert kinds["guidance"] is ctypes.c_float and kinds["rescale"] is ctypes.c_float
    for ptr in ("eps", "guidance_rows", "rescale_rows"):
        assert kinds[ptr] is ctypes.c_void_p, ptr


def test_no_step_block_grew():
    """the rescale is a launch of its own: the parameter blocks of the eight step entry points are what they were"""
    from imagdressing_amd import _lib
    for cname, py, size, last in (("imd_sampler_params", _lib.SamplerParams, 168, "coefs"), ("imd_unipc_params", _lib.UnipcParams, 184, "coefs"),
                                  ("imd_ddim_params", _lib.DdimParams, 128, "sigma")):
        names = [f[0] for f in py._fields_]
        assert names == header_struct_fields(cname)
        assert names[-1] == last and not any("rescale" in n for n in names)
        assert ctypes.sizeof(py) == size, (cname, ctypes.sizeof(py))


def test_foreign_struct_size_and_null_params_are_refused(lib):
    from imagdressing_amd import _lib
    p = _lib.GuidanceRescaleParams()
    assert p.struct_bytes == ctypes.sizeof(_lib.GuidanceRescaleParams)
    for bad in (p.struct_bytes - 8, p.struct_bytes + 8, ctypes.sizeof(_lib.SamplerParams), 0):
        q = _lib.GuidanceRescaleParams()
        q.struct_bytes = bad            # eps is NULL: a library that read on would answer "null eps" instead
        assert lib.imd_guidance_rescale(ctypes.byref(q), None) != 0
        assert lib.imd_last_error().startswith(b"guidance_rescale:") and b"parameter block is" in lib.imd_last_error()
    assert lib.imd_guidance_rescale(None, None) != 0 and b"guidance_rescale: null params" in lib.imd_last_error()
    assert lib.imd_guidance_rescale(ctypes.byref(p), None) != 0 and b"guidance_rescale: null eps" in lib.imd_last_error()


REFUSALS = [(dict(eps=None), b"null eps"), (dict(eps=0x1008), b"eps must be 16-byte aligned"), (dict(eps=0x1004), b"16-byte"),
            (dict(guidance_rows=0x2002), b"4-byte aligned"), (dict(rescale_rows=0x3001), b"4-byte aligned"),
            (dict(B=0), b"empty latent"), (dict(B=-1), b"empty latent"), (dict(HW=0), b"empty latent"),
            (dict(rescale=float("nan")), b"rescale"), (dict(rescale=float("inf")), b"rescale"), (dict(rescale=-0.1), b"in [0, 1]"),
            (dict(rescale=1.5), b"in [0, 1]"), (dict(guidance=float("nan")), b"guidance ("), (dict(guidance=float("inf")), b"must be finite"),
            (dict(guidance=-float("inf")), b"must be finite")]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_launcher_refusals_precede_the_launch(lib, case):
    over, word = REFUSALS[case]
    p = launchable_block()
    for k, v in over.items():
        setattr(p, k, v)
    assert lib.imd_guidance_rescale(ctypes.byref(p), None) != 0
    err = lib.imd_last_error()
    assert err.startswith(b"guidance_rescale:") and word in err and b"launch failed" not in err, err


def test_a_scalar_zero_launches_nothing(lib):
    """rescale = 0 for every row: success without a device (nothing is launched, eps is not dereferenced)"""
    p = launchable_block()
    p.rescale = 0.0
    assert lib.imd_guidance_rescale(ctypes.byref(p), None) == 0


def test_the_wrapper_has_no_cpu_path():
    import torch
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    with pytest.raises(ImdError):
        ops.guidance_rescale(torch.zeros(4, 4, 4), guidance=7.5, rescale=0.7)
    with pytest.raises(ImdError):
        ops.guidance_rescale(torch.zeros(4, 4, 4), guidance=torch.ones(2), rescale=torch.ones(2))
