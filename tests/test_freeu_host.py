"""FreeU on the host: the closed form against the FFT form, the preconditions and the sensitivity of the exact GPU comparison
(tests/test_freeu_gpu.py), the validation of ``enable_freeu`` on the UNet and the pipelines, and the refusals of ``imd_concat2_freeu``
(they precede any launch, so the library answers them without a GPU)."""
import ctypes
import os

import pytest
import torch

from tests import exact_cases as ec
from tests import freeu_oracle as fo

F64 = torch.float64
DTS = (torch.bfloat16, torch.float16)


def test_closed_form_equals_fft_form():
    g = torch.Generator().manual_seed(0)
    for H, W in fo.MAP_SIZES:
        x = torch.randn(2, 3, H, W, generator=g, dtype=F64)
        for s in (0.9, 0.2, 0.5):
            err = float((fo.closed_form(x, s) - fo.fourier_filter_ref(x, 1, s)).abs().max())
            assert err <= 1e-12, f"{H} x {W}, scale {s}: closed form off by {err:.3g}"


def test_indicator_maps_have_the_stated_factors():
    for name, (m, factor) in fo.indicator_maps().items():
        assert set(m.unique().tolist()) <= {-2.0, 0.0, 2.0} and float(m.abs().max()) == 2.0
        got = fo.fourier_filter_ref(m, 1, fo.EXACT_SKIP_SCALE)
        assert float((got - factor * m).abs().max()) < 1e-12, name


def test_exact_cases_meet_their_preconditions():
    """Every expected output is a multiple of 1/16 that bf16 AND fp16 hold exactly, and every (image, group) sum and sum of squares,
    times 256, stays below 2^24: the fp32 partials are exact in any order."""
    cases = fo.exact_cases()
    assert {(c[1], c[2]) for c in cases} == set(fo.EXACT_MAPS) | {fo.AWKWARD[:2]} and {c[0] for c in cases} == {1, 3}
    for case in cases:
        B, H, W, Ca, Cb, G, ctrl = case
        a, b, add = fo.exact_operands(case)
        assert (add is not None) == ctrl
        for t in (a, b) + (() if add is None else (add,)):
            assert set(t.unique().tolist()) <= {-2.0, 0.0, 2.0}
        if add is not None:
            assert float((b + add).abs().max()) <= 4.0
        for dt in DTS:
            want = fo.exact_expected(case, a, b, add, dt)
            assert torch.equal(want.to(dt).to(F64), want), f"{case} {dt}: an expected output is not representable"
        sums, _ = ec.group_sums(want, G)
        assert float(sums.abs().max()) * 256 < ec.EXACT_BELOW, case
        assert torch.equal(sums * 256, (sums * 256).round())


def _differs(case, dt, **mutation):
    a, b, add = fo.exact_operands(case)
    want = fo.exact_expected(case, a, b, add, dt)
    mut, _ = fo.concat_freeu_ref(a, b, add, fo.EXACT_BACKBONE_SCALE, fo.EXACT_SKIP_SCALE, dt, **mutation)
    # what a kernel with the mutation would store: its exact value (a dyadic rational here -- the float64 noise of the FFT is snapped away
    # first, or a 1e-17 in place of a 0 would count as a difference), rounded to the element type
    snapped = (mut * 4096).round() / 4096
    assert float((mut - snapped).abs().max()) < 1e-9
    return not torch.equal(snapped.to(dt), want.to(dt))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
def test_exact_comparison_catches_each_mutation(dt):
    cases = fo.exact_cases()
    four = [c for c in cases if (c[1], c[2]) == (4, 4)]
    assert len(four) == 8
    # the closed form itself passes the comparison everywhere: the mutations below are what fails it
    assert not any(_differs(c, dt, closed=True) for c in cases)
    assert all(_differs(c, dt, anti=True) for c in four), "anti-diagonal wave in place of the diagonal"
    one_row = [c for c in cases if c[1] == 1]
    assert len(one_row) == 16 and all(_differs(c, dt, double=True) for c in one_row), "a frequency counted twice on one-row maps"
    x = torch.randn(1, 1, 5, 1, dtype=F64, generator=torch.Generator().manual_seed(3))
    assert float((fo.closed_form(x, 0.5, double=True) - fo.fourier_filter_ref(x, 1, 0.5)).abs().max()) > 1e-3     # ... and on one-column maps
    assert all(_differs(c, dt, drop_add=True) for c in four if c[6]), "b_add dropped"
    assert all(_differs(c, dt, upper=True) for c in four), "the upper backbone half scaled"
    assert all(_differs(c, dt, filter_backbone_channel=ch) for c in four for ch in (0, c[3] - 1)), "a backbone channel filtered"
    assert all(_differs(c, dt, skip_unfiltered=ch) for c in four for ch in (0, c[4] - 1)), "a skip channel left unfiltered"


# ---- enable_freeu -----------------------------------------------------------------------------------------------------------------------------------
def _bare_unet(n_up=4):
    from imagdressing_amd.unet import UNet2DConditionModel
    u = object.__new__(UNet2DConditionModel)
    u.up_blocks = [object()] * n_up
    return u


def test_unet_enable_freeu_validation():
    u = _bare_unet()
    assert getattr(u, "_freeu", None) is None
    assert u.enable_freeu(0.9, 0.2, 1.5, 1.6) is u
    assert u._freeu == ((1.5, 0.9), (1.6, 0.2))              # (backbone, skip) of up_blocks[0], of up_blocks[1]
    assert u.disable_freeu() is u and u._freeu is None
    for k in range(4):
        for bad in (0, 0.0, -1.0, float("nan"), float("inf"), None, "1", True):
            args = [0.9, 0.2, 1.5, 1.6]
            args[k] = bad
            with pytest.raises(ValueError, match=("s1", "s2", "b1", "b2")[k]):
                u.enable_freeu(*args)
            assert u._freeu is None                            # a refused call leaves the switch as it was
    with pytest.raises(ValueError, match="up blocks"):
        _bare_unet(2).enable_freeu(0.9, 0.2, 1.5, 1.6)


def test_pipelines_delegate_to_the_unet():
    from imagdressing_amd import scheduler as S
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline as base
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet as ctrl
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet_inpainting as inp
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_ipa_controlnet as ipa
    kw = dict(vae=None, reference_unet=None, tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None)
    sch = lambda: S.DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",    # noqa: E731
                                  clip_sample=False, set_alpha_to_one=False, steps_offset=1)
    def make(mod, unet, ref):
        if mod is ipa:                          # (its constructor builds the face projection from the UNet's config: bare instance instead)
            pipe = object.__new__(mod.IMAGDressing_v1)
            pipe.unet, pipe.reference_unet = unet, ref
            return pipe
        extra = {} if mod is base else {"controlnet": None}
        return mod.IMAGDressing_v1(unet=unet, scheduler=sch(), **extra, **dict(kw, reference_unet=ref))
    for mod in (base, ctrl, inp, ipa):
        pipe = make(mod, None, None)
        for call in (lambda: pipe.enable_freeu(0.9, 0.2, 1.5, 1.6), pipe.disable_freeu):
            with pytest.raises(ValueError, match="no unet"):
                call()
        u, ref = _bare_unet(), _bare_unet()
        pipe = make(mod, u, ref)
        assert pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=1.6) is pipe
        assert u._freeu == ((1.5, 0.9), (1.6, 0.2)) and getattr(ref, "_freeu", None) is None       # the garment UNet is untouched
        with pytest.raises(ValueError, match="b2"):
            pipe.enable_freeu(0.9, 0.2, 1.5, 0)
        assert pipe.disable_freeu() is pipe and u._freeu is None


# ---- the C entry point's refusals ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# name -> (overrides of the good call, a word of the message).  Shared with tests/test_freeu_gpu.py, which checks that nothing was launched.
REFUSALS = {
    "null a": (dict(a=None), "null pointer"), "null b": (dict(b=None), "null pointer"), "null out": (dict(out=None), "null pointer"),
    "Ca % 16": (dict(Ca=24), "multiple of 16"), "Cb % 8": (dict(Cb=12), "multiple of 16"),
    "H < 1": (dict(H=0), "empty tensor"), "W < 1": (dict(W=0), "empty tensor"), "B < 1": (dict(B=0, b_batch=0), "empty tensor"),
    "H above the table": (dict(H=257), "twiddle table"), "W above the table": (dict(W=257), "twiddle table"),
    "b_batch != B": (dict(b_batch=1), "b_batch"),
    "(Ca + Cb) % G": (dict(G=5), "multiple of G"),
    "dtype": (dict(dtype=2), "unknown dtype"),
    "misaligned a": (dict(a_off=8), "misaligned"), "misaligned b": (dict(b_off=2), "misaligned"), "misaligned b_add": (dict(add_off=4), "misaligned"),
    "misaligned out": (dict(out_off=8), "misaligned"),
    "backbone_scale 0": (dict(backbone_scale=0.0), "finite and > 0"), "backbone_scale nan": (dict(backbone_scale=float("nan")), "finite and > 0"),
    "skip_scale negative": (dict(skip_scale=-0.5), "finite and > 0"), "skip_scale inf": (dict(skip_scale=float("inf")), "finite and > 0"),
}


def call_with(lib, ptrs, over, stream=None):
    """``imd_concat2_freeu`` on the good call (B 2, 4 x 4, 32 + 16 channels, G 4, bf16) with ``over`` applied; ptrs: a, b, add, out, part."""
    kw = dict(a=ptrs["a"], b=ptrs["b"], add=ptrs["add"], out=ptrs["out"], part=ptrs["part"], Ca=32, Cb=16, B=2, H=4, W=4, b_batch=2, G=4,
              backbone_scale=1.5, skip_scale=0.5, dtype=0, a_off=0, b_off=0, add_off=0, out_off=0)
    kw.update(over)
    off = lambda p, o: None if p is None else p + o            # noqa: E731
    return lib.imd_concat2_freeu(off(kw["a"], kw["a_off"]), kw["Ca"], off(kw["b"], kw["b_off"]), kw["Cb"], off(kw["add"], kw["add_off"]),
                                 off(kw["out"], kw["out_off"]), kw["B"], kw["H"], kw["W"], kw["b_batch"], kw["G"], kw["part"],
                                 kw["backbone_scale"], kw["skip_scale"], kw["dtype"], stream)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_point_refusals_precede_the_launch(lib, name):
    """Host buffers stand in for the device tensors: a refused call never reads them (and never reaches the GPU runtime)."""
    bufs = {k: ctypes.create_string_buffer(4096 + 64) for k in ("a", "b", "add", "out", "part")}
    ptrs = {k: (ctypes.addressof(v) + 63) // 64 * 64 for k, v in bufs.items()}
    over, word = REFUSALS[name]
    assert call_with(lib, ptrs, over) != 0
    msg = lib.imd_last_error().decode()
    assert msg.startswith("concat2 + freeu:") and word in msg, msg
    assert bufs["out"].raw == bytes(4096 + 64)


def test_parts_query(lib):
    q = lib.imd_concat2_freeu_parts
    assert q(2, 8, 10, 1280, 1280, 32) == 3 and q(2, 16, 20, 1280, 640, 32) == 3 and q(2, 4, 4, 16, 16, 4) == 1
    assert q(1, 2, 2, 32, 16, 4) == 2                       # 12 channels per group: group 2 (24 .. 35) lies in two workgroups
    assert q(2, 8, 8, 64, 64, 32) == 1                      # 4 channels per group
    for bad in ((0, 4, 4, 16, 16, 4), (1, 0, 4, 16, 16, 4), (1, 4, 4, 24, 16, 4), (1, 4, 4, 16, 12, 4), (1, 4, 4, 16, 16, 5), (1, 4, 4, 16, 16, 0),
                (1, 4, 4, 320, 320, 128), (1, 4, 4, 32, 16, 8)):          # ... G > 64; 6 channels per group
        assert q(*bad) == 0, bad
