"""FreeU inside the skip concatenation (``imd_concat2_freeu``, ``ops.concat_channels_freeu``, ``enable_freeu``) on the GPU, bf16 and fp16.

Exact family -- maps whose twiddles are all 0 or +-1 (4x4, 2x4, 2x2, 1x2, 1x1), data in {-2, 0, 2}, skip_scale 0.5, backbone_scale 1.5:
every output is a multiple of 1/16 (tests/test_freeu_host.py asserts the preconditions and that the comparison catches six mutations), so
the stored tensor EQUALS the float64 reference and the fp32 statistic partials, folded in float64, EQUAL the exact sums.
Parity family -- Gaussian data against the float64 FFT restatement (tests/freeu_oracle.py), one ulp of the element type plus an fp32 term.
Identities, refusals, the UNet against the oracle with FreeU installed, the pipelines."""
import pytest
import torch

from tests import exact_cases as ec
from tests import freeu_oracle as fo
from tests.test_freeu_host import REFUSALS, call_with

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTS = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
EPS = 1e-5
FREEU = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def dev(t, dt=None):
    return None if t is None else (t if dt is None else t.to(dt)).to("cuda")


def launch(ops, a, b, add, bs, ss, dt, G=0):
    return ops.concat_channels_freeu(dev(a, dt), dev(b, dt), dev(add, dt), a.shape[1], a.shape[2], bs, ss, gn_stats_groups=G)


# ---- exact family -------------------------------------------------------------------------------------------------------------------------------
def check_exact(ops, out, want, G, dt, what):
    """The stored tensor, the carried partials (exact), and GroupNorm from them against a statistics launch on the stored tensor."""
    B, H, W, C = want.shape
    bad = out.cpu() != want.to(dt)
    assert out.dtype == dt and not bool(bad.any()), f"{what}: {int(bad.sum())} stored elements differ, first at {bad.nonzero()[0].tolist()}"
    st = getattr(out, "_imd_gn_stats", None)
    assert st is not None and st[2] == G, f"{what}: the launch must hand its statistics on"
    part, nparts, _ = st
    assert part.dtype == torch.float32 and tuple(part.shape) == (B, nparts, G, 2)
    exact, _ = ec.group_sums(want, G)
    got = part.to(F64).sum(1).cpu()
    assert torch.equal(got, exact), f"{what}: {int((got != exact).sum())} of {exact.numel()} folded statistics differ from the exact sums"
    # consumers: coefficients within 1e-5, the normalised output within one 16-bit ulp (the bars of tests/test_gn_statistics_exact_gpu.py)
    gamma, beta = ec.away_from_zero_affine(7, C)
    x3 = out.view(B, H * W, C)
    x3._imd_gn_stats = st
    plain = x3.clone()
    assert getattr(plain, "_imd_gn_stats", None) is None
    a1, b1 = ops.group_norm_coeffs(x3, dev(gamma), dev(beta), groups=G, eps=EPS)
    a2, b2 = ops.group_norm_coeffs(plain, dev(gamma), dev(beta), groups=G, eps=EPS)
    a1, b1, a2, b2 = (t.to(F64).cpu() for t in (a1, b1, a2, b2))
    ref = ec.gn_reference(want.view(B, H * W, C), G, gamma, beta, EPS)
    rel = ((a1 - a2).abs() / a2.abs()).max().item()
    slack = ((b1 - b2).abs() / (beta.to(F64).abs() + ref["mean_a"].abs())).max().item()
    assert rel <= 1e-5 and slack <= 1e-5, f"{what}: coefficients from the carried statistics off by {rel:.3g} / {slack:.3g}"
    y1 = ops.group_norm(x3, dev(gamma), dev(beta), groups=G, eps=EPS, silu=True)
    y2 = ops.group_norm(plain, dev(gamma), dev(beta), groups=G, eps=EPS, silu=True)
    err = (y1.to(F64) - y2.to(F64)).abs().cpu() / ec.ulp_at(y2.to(F64).cpu(), dt)
    assert bool((err <= 1.0).all()), f"{what}: normalised output {err.max().item():.3f} ulp from the two-launch form"


@pytest.mark.parametrize("case", fo.exact_cases(), ids=str)
@DTS
def test_exact_cases(ops, case, dt):
    B, H, W, Ca, Cb, G, ctrl = case
    a, b, add = fo.exact_operands(case)
    want = fo.exact_expected(case, a, b, add, dt)
    out = launch(ops, a, b, add, fo.EXACT_BACKBONE_SCALE, fo.EXACT_SKIP_SCALE, dt, G)
    assert out._imd_gn_stats[1] == ops.L.load().imd_concat2_freeu_parts(B, H, W, Ca, Cb, G)
    check_exact(ops, out, want, G, dt, f"concat2_freeu_kernel {case}")


@pytest.mark.parametrize("Ca,Cb,G", fo.EXACT_LAYOUTS)
@pytest.mark.parametrize("name", sorted(fo.indicator_maps()))
@DTS
def test_indicator_maps(ops, name, Ca, Cb, G, dt):
    """A constant map x 0.5, the diagonal wave x 0.75, the anti-diagonal wave unchanged, the row wave x 0.75 -- in every skip channel
    beside a random backbone, then alone in one skip channel with every other channel zero."""
    m, factor = fo.indicator_maps()[name]
    B = 2
    g = torch.Generator().manual_seed(5)
    a = (torch.randint(-1, 2, (B, 4, 4, Ca), generator=g) * 2).to(F64)
    b = m[None, :, :, None].expand(B, 4, 4, Cb).contiguous()
    back = a.clone()
    back[..., :Ca // 2] *= fo.EXACT_BACKBONE_SCALE
    out = launch(ops, a, b, None, fo.EXACT_BACKBONE_SCALE, fo.EXACT_SKIP_SCALE, dt, G)
    check_exact(ops, out, torch.cat([back, factor * b], -1), G, dt, f"{name} in every skip channel")
    for c in (0, 5, Cb - 1):
        one = torch.zeros(B, 4, 4, Cb, dtype=F64)
        one[1, :, :, c] = m
        out = launch(ops, torch.zeros_like(a), one, None, fo.EXACT_BACKBONE_SCALE, fo.EXACT_SKIP_SCALE, dt, G)
        check_exact(ops, out, torch.cat([torch.zeros_like(a), factor * one], -1), G, dt, f"{name} alone in skip channel {c}")


# ---- parity family ------------------------------------------------------------------------------------------------------------------------------
PARITY_MAPS = [(3, 5), (6, 10), (8, 10), (16, 20), (32, 40), (5, 1)]
PARITY_CHANNELS = [(320, 320, 8), (320, 160, 8), (1280, 1280, 32)]
# The fp32 term of the bound: 4 x the largest excess of |stored - float64 reference| over one ulp of the element type at |reference|, measured over
# every case of test_parity_against_float64 on an MI355X (each run prints its own): 2.08e-8, at fp16 (the largest bf16 excess is negative, -2.2e-7:
# no bf16 element reaches one ulp).  2^-14 max|v| is 2.9e-4 .. 4.1e-4 over these cases, over three thousand times the term.
MEASURED_EXCESS = 2.08e-8
FP32_TERM = 4 * MEASURED_EXCESS


def parity_case(ops, H, W, Ca, Cb, G, s, bsc, dt):
    """-> (largest excess of |stored - float64 reference| over one ulp of ``dt`` at |reference|, 2^-14 max|v|, the stored tensor)"""
    B = 2
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + Ca + Cb)
    a, b, add = (torch.randn(B, H, W, c, generator=g).to(dt) for c in (Ca, Cb, Cb))
    ref, v = fo.concat_freeu_ref(a, b, add, fo.f32(bsc), fo.f32(s), dt)
    out = launch(ops, a, b, add, bsc, s, dt, G)
    err = (out.to(F64).cpu() - ref).abs()
    excess = float((err - fo.ulp_at(ref, dt)).max())
    cap = 2.0 ** -14 * float(v.abs().max())
    print(f"freeu parity {H}x{W} {Ca}+{Cb} s={s} b={bsc} {dt}: max err {float(err.max()):.3e}, excess over one ulp {excess:.3e}, 2^-14 max|v| = {cap:.3e}")
    return excess, cap, out


@pytest.mark.parametrize("s,bsc", [(0.9, 1.5), (0.2, 1.6)])
@pytest.mark.parametrize("Ca,Cb,G", PARITY_CHANNELS)
@pytest.mark.parametrize("H,W", PARITY_MAPS)
@DTS
def test_parity_against_float64(ops, H, W, Ca, Cb, G, s, bsc, dt):
    """Gaussian a, b, b_add of std 1, B = 2, against the float64 FFT restatement fed the same 16-bit inputs, v = round16(b + b_add) and the
    fp32 values of the two scales.  Bound per element: one ulp of the element type at |ref| (the final rounding, and the reference sitting
    just across a binade) + FP32_TERM for the seven fp32 sums; FP32_TERM must stay below 2^-14 max|v| -- above that the sums are not being
    accumulated in fp32.  Measured on an MI355X: largest excess 2.08e-8 (fp16, 5 x 1, 320 + 320, s = 0.2); FP32_TERM = 8.3e-8."""
    excess, cap, out = parity_case(ops, H, W, Ca, Cb, G, s, bsc, dt)
    assert FP32_TERM < cap
    assert excess <= FP32_TERM, f"an element lies {excess:.3e} beyond one ulp, the fp32 term allows {FP32_TERM:.3g}"
    # the statistics describe the stored tensor: fp32 sums against float64 sums of the same values.  A thread adds at most 20 pixels x 8 channels
    # in sequence and the rest is a tree of about 12 levels: at most (160 + 12) 2^-24 = 1.03e-5 of the sum of magnitudes, which is Q itself
    # for Q and at most (Q + n) / 2 for S -> 2e-5 (Q + n) bounds both
    exact, n = ec.group_sums(out.to(F64).cpu(), G)
    got = out._imd_gn_stats[0].to(F64).sum(1).cpu()
    assert bool(((got - exact).abs() <= 2e-5 * (exact[..., 1:2] + n)).all())


# ---- identities ---------------------------------------------------------------------------------------------------------------------------------
def gauss(seed, B, H, W, Ca, Cb, dt):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, W, c, generator=g).to(dt) for c in (Ca, Cb, Cb))


@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "b_add"])
@DTS
def test_unit_scales_store_the_plain_concatenation(ops, dt, ctrl):
    a, b, add = gauss(1, 2, 8, 10, 320, 160, dt)
    add = add if ctrl else None
    want = ops.concat_channels(dev(a), dev(b), dev(add), gn_stats_groups=8)
    out = launch(ops, a, b, add, 1.0, 1.0, dt, 8)
    assert torch.equal(out, want)
    assert torch.equal(launch(ops, a, b, add, 1.0, 1.0, dt, 0), want) and not torch.equal(launch(ops, a, b, add, 1.0, 0.9, dt, 8), want)
    assert not torch.equal(launch(ops, a, b, add, 1.5, 1.0, dt, 8), want)
    # ... and GroupNorm of it from the carried statistics is within one ulp of GroupNorm from concat_channels' statistics
    gamma, beta = ec.away_from_zero_affine(7, 480)
    y1 = ops.group_norm(out, dev(gamma), dev(beta), groups=8, eps=EPS, silu=True)
    y2 = ops.group_norm(want, dev(gamma), dev(beta), groups=8, eps=EPS, silu=True)
    assert bool(((y1.to(F64) - y2.to(F64)).abs().cpu() <= ec.ulp_at(y2.to(F64).cpu(), dt)).all())


@DTS
def test_images_of_a_batch_are_independent(ops, dt):
    a, b, add = gauss(2, 3, 6, 10, 320, 160, dt)
    out = launch(ops, a, b, add, 1.5, 0.9, dt, 8)
    for r in range(3):
        solo = launch(ops, a[r:r + 1], b[r:r + 1], add[r:r + 1], 1.5, 0.9, dt, 8)
        assert torch.equal(out[r:r + 1], solo), r
        assert torch.equal(out._imd_gn_stats[0][r:r + 1], solo._imd_gn_stats[0])


@DTS
def test_nothing_is_written_past_out_or_part(ops, dt):
    """out and part sit inside larger buffers filled with a sentinel: the bytes behind them (and in front) are untouched."""
    B, H, W, Ca, Cb, G = 2, 6, 10, 320, 160, 8
    a, b, add = gauss(3, B, H, W, Ca, Cb, dt)
    lib = ops.L.load()
    n_out, nparts = B * H * W * (Ca + Cb), lib.imd_concat2_freeu_parts(B, H, W, Ca, Cb, G)
    n_part = B * nparts * G * 2
    pad = 256
    obuf = torch.full((n_out + 2 * pad,), 0x5A5A, dtype=torch.int16, device="cuda")
    pbuf = torch.full((n_part + 2 * pad,), -12345.0, dtype=torch.float32, device="cuda")
    da, db, dadd = dev(a), dev(b), dev(add)
    rc = lib.imd_concat2_freeu(da.data_ptr(), Ca, db.data_ptr(), Cb, dadd.data_ptr(), obuf.data_ptr() + 2 * pad, B, H, W, B, G,
                               pbuf.data_ptr() + 4 * pad, 1.5, 0.9, ops.DTYPE_CODE[dt], ops._stream())
    assert rc == 0, lib.imd_last_error()
    torch.cuda.synchronize()
    want = launch(ops, a, b, add, 1.5, 0.9, dt, G)
    assert torch.equal(obuf[pad:pad + n_out].view(dt).view(B, H, W, Ca + Cb), want)
    assert torch.equal(pbuf[pad:pad + n_part].view(B, nparts, G, 2), want._imd_gn_stats[0])
    assert bool((obuf[:pad] == 0x5A5A).all()) and bool((obuf[pad + n_out:] == 0x5A5A).all())
    assert bool((pbuf[:pad] == -12345.0).all()) and bool((pbuf[pad + n_part:] == -12345.0).all())


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_launch_nothing(ops, name):
    lib = ops.L.load()
    bufs = {k: torch.full((8192,), 0x5A5A, dtype=torch.int16, device="cuda") for k in ("a", "b", "add", "out", "part")}
    over, word = REFUSALS[name]
    rc = call_with(lib, {k: v.data_ptr() for k, v in bufs.items()}, over, stream=ops._stream())
    msg = lib.imd_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith("concat2 + freeu:") and word in msg, msg
    assert bool((bufs["out"] == 0x5A5A).all()) and bool((bufs["part"] == 0x5A5A).all())


def test_the_good_call_of_the_refusal_table_is_accepted(ops):
    lib = ops.L.load()
    bufs = {k: torch.zeros(8192, dtype=torch.int16, device="cuda") for k in ("a", "b", "add", "out", "part")}
    assert call_with(lib, {k: v.data_ptr() for k, v in bufs.items()}, {}, stream=ops._stream()) == 0, lib.imd_last_error()
    torch.cuda.synchronize()


def test_ops_refuses_what_the_launch_cannot_take(ops):
    a, b, add = gauss(4, 2, 4, 4, 32, 16, torch.float16)
    with pytest.raises(ops.L.ImdError, match="one B"):
        ops.concat_channels_freeu(dev(a), dev(b[:1]), None, 4, 4, 1.5, 0.9)          # a half-batch skip
    with pytest.raises(ops.L.ImdError, match="finite and > 0"):
        ops.concat_channels_freeu(dev(a), dev(b), None, 4, 4, 0.0, 0.9)
    # where the statistics conditions do not hold the launch writes none and group_norm runs its own pass
    out = ops.concat_channels_freeu(dev(a), dev(b), None, 4, 4, 1.5, 0.9, gn_stats_groups=5)
    assert getattr(out, "_imd_gn_stats", None) is None
    assert torch.equal(out, ops.concat_channels_freeu(dev(a), dev(b), None, 4, 4, 1.5, 0.9, gn_stats_groups=4))


# ---- UNet ---------------------------------------------------------------------------------------------------------------------------------------
def g(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


UNET_BARS = {torch.float16: dict(rel_rms=5e-3, max_rel=2e-2), torch.bfloat16: dict(rel_rms=2.5e-2, max_rel=0.12)}      # test_full_width_unet_forward_vs_oracle's


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def pair(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.harness import SMALL, build_pair
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=request.param)
    p["dtype"] = request.param
    return p


def _garment(p, lh, lw):
    from imagdressing_amd.unet import nchw_to_nhwc8
    from oracle.pipeline import garment_features
    refl, cloth = g(13, 1, 4, lh, lw), g(12, 2, 16, 64, scale=0.5)
    sa_o = garment_features(p["o_ref"], refl, cloth)
    p["e_ref"].forward_nhwc(nchw_to_nhwc8(refl.cuda(), p["dtype"]), 0, cloth[1:2].cuda().to(p["dtype"]).contiguous())
    return sa_o, {n: pr.cache["hidden_states"].clone() for n, pr in p["e_ref"].attn_processors.items()}


@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlnet"])
@pytest.mark.parametrize("lh,lw", [(24, 40), (16, 32)])
@torch.no_grad()
def test_unet_forward_with_freeu_vs_oracle(pair, lh, lw, ctrl):
    """SMALL UNet, FreeU (0.9, 0.2, 1.5, 1.6) on both sides; latents 24 x 40 (concat sites 3 x 5 and 6 x 10) and 16 x 32 (2 x 4 and 4 x 8); the
    CFG batch [cond; uncond] at t = 481 against the oracle's cond and plain passes; with a ControlNet the residuals reach the filter through
    b_add and the oracle adds them to its skips.  Bars: test_full_width_unet_forward_vs_oracle's.  disable_freeu() restores the pre-enable
    output bit for bit, and the switch really changes the result (it moves the oracle's own output by 46 - 48 % rms).  Measured on an MI355X
    (rel_rms / max_abs over ref_std for the cond and the uncond row; each run prints its own):
      fp16  24x40  plain       2.22e-3 / 1.05e-2   1.87e-3 / 7.8e-3      bf16  24x40  plain       1.72e-2 / 6.2e-2   1.51e-2 / 6.3e-2
            24x40  controlnet  2.22e-3 / 9.0e-3    1.93e-3 / 1.08e-2            24x40  controlnet  1.77e-2 / 7.1e-2   1.50e-2 / 6.7e-2
            16x32  plain       2.16e-3 / 8.4e-3    2.01e-3 / 7.0e-3             16x32  plain       1.71e-2 / 9.4e-2   1.56e-2 / 6.1e-2
            16x32  controlnet  2.21e-3 / 9.6e-3    1.96e-3 / 7.2e-3             16x32  controlnet  1.71e-2 / 6.5e-2   1.58e-2 / 7.5e-2"""
    from imagdressing_amd.unet import nchw_to_nhwc8
    from tests.harness import err_stats
    p, dt = pair, pair["dtype"]
    sa_o, sa_e = _garment(p, lh, lw)
    lat, ehs = g(100, 1, 4, lh, lw), g(101, 1, 77, 64, scale=0.5)
    pose = torch.rand(1, 3, 8 * lh, 8 * lw, generator=torch.Generator().manual_seed(103))
    x2, ehs2 = nchw_to_nhwc8(lat.repeat(2, 1, 1, 1).cuda(), dt), ehs.repeat(2, 1, 1).cuda().to(dt).contiguous()
    cak = {"sa_hidden_states": sa_e, "sa_batch_mask": torch.tensor([1.0, 0.0], device="cuda")}

    def engine():
        down = mid = None
        if ctrl:
            down, mid = p["e_ctrl"].forward_nhwc(x2, 481, ehs2, nchw_to_nhwc8(pose.cuda(), dt), 0.8)
        return p["e_unet"].forward_nhwc(x2, 481, ehs2, cak, down, mid).view(2, lh, lw, 4).permute(0, 3, 1, 2).clone()
    off = engine()
    assert p["e_unet"].enable_freeu(**FREEU) is p["e_unet"]
    try:
        on = engine()
    finally:
        p["e_unet"].disable_freeu()
    assert torch.equal(engine(), off), "disable_freeu() must restore the pre-enable output bit for bit"
    assert torch.isfinite(on).all() and not torch.equal(on, off)
    kw = {}
    if ctrl:
        down_o, mid_o = p["o_ctrl"](lat, 481, ehs, pose, 0.8)
        kw = dict(down_block_additional_residuals=down_o, mid_block_additional_residual=mid_o)
    fo.install_freeu(p["o_unet"], **FREEU)
    try:
        ref_c = p["o_unet"](lat, 481, ehs, cross_attention_kwargs={"sa_hidden_states": sa_o}, **kw)
        ref_u = p["o_unet"](lat, 481, ehs, **kw)
    finally:
        fo.uninstall_freeu(p["o_unet"])
    ref_off = p["o_unet"](lat, 481, ehs, **kw)
    bar = UNET_BARS[dt]
    moved = err_stats(ref_u, ref_off)["rel_rms"]
    for name, got, ref in (("cond", on[0:1], ref_c), ("uncond", on[1:2], ref_u)):
        st = err_stats(got, ref)
        print(f"freeu unet {lh}x{lw} ctrl={ctrl} {dt} {name}: rel_rms {st['rel_rms']:.3e} max_abs/ref_std {st['max_abs'] / st['ref_std']:.3e} "
              f"(the switch moves the oracle by rel_rms {moved:.3e})")
        assert st["rel_rms"] < bar["rel_rms"] and st["max_abs"] < bar["max_rel"] * st["ref_std"], st
    assert moved > 3 * bar["rel_rms"], f"FreeU moves the oracle's output by only {moved:.3e}: the comparison above could not tell it from off"


# ---- pipelines ----------------------------------------------------------------------------------------------------------------------------------
STEPS = 4


def _pipe(p, name="ddim"):
    from imagdressing_amd import scheduler as S
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    sch = (S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kw) if name == "ddim" else S.DPMSolverMultistepScheduler(**kw))
    return IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           image_encoder=None, ImgProj=lambda h: h, scheduler=sch, safety_checker=None, feature_extractor=None)


@pytest.mark.parametrize("name", ["ddim", "dpm"])
@torch.no_grad()
def test_pipeline_switch_changes_the_latents_and_replays_under_a_step_graph(pair, name):
    from tests.test_multi_request_gpu import _Requests
    p, reqs = pair, _Requests(R=1)
    pipe = _pipe(p, name)
    kw = lambda: dict(num_inference_steps=STEPS, **reqs.solo_kwargs(0))          # noqa: E731
    off = pipe(**kw()).images
    assert pipe.enable_freeu(**FREEU) is pipe
    try:
        on = pipe(**kw()).images
        assert torch.isfinite(on).all() and not torch.equal(on, off)
        pipe.enable_step_graph(True)
        try:
            graph = pipe(**kw()).images
            assert getattr(pipe, "_last_step_graph", None) is not None
        finally:
            pipe.enable_step_graph(False)
        assert torch.equal(graph, on), (graph - on).abs().max().item()
    finally:
        pipe.disable_freeu()
    assert torch.equal(pipe(**kw()).images, off)


@torch.no_grad()
def test_pipeline_solo_call_equals_its_rows_of_a_request_batch(pair):
    from tests.test_multi_request_gpu import _Requests
    p, reqs = pair, _Requests(R=2)
    pipe = _pipe(p).enable_freeu(**FREEU)
    try:
        both = pipe(num_inference_steps=STEPS, **reqs.call_kwargs()).images
        for r in range(2):
            solo = pipe(num_inference_steps=STEPS, **reqs.solo_kwargs(r)).images
            assert torch.equal(both[r:r + 1], solo), (r, (both[r:r + 1] - solo).abs().max().item())
    finally:
        pipe.disable_freeu()


@torch.no_grad()
def test_deepcache_runs_the_freeu_launch_on_full_steps_only(pair, ops):
    from imagdressing_amd.dressing_sd.pipelines._base import deepcache_plan
    from tests.test_multi_request_gpu import _Requests
    p, reqs = pair, _Requests(R=1)
    pipe = _pipe(p).enable_freeu(**FREEU)
    try:
        n0 = ops.FREEU_COUNTER["launches"]
        plain = pipe(num_inference_steps=STEPS, **reqs.solo_kwargs(0)).images
        assert ops.FREEU_COUNTER["launches"] - n0 == 6 * STEPS                       # three resnets in each of the two blocks, every step
        pipe.enable_deepcache(2)
        n0 = ops.FREEU_COUNTER["launches"]
        cached = pipe(num_inference_steps=STEPS, **reqs.solo_kwargs(0)).images
        plan = deepcache_plan(STEPS, 2)
        assert plan == [True, False, True, False] and ops.FREEU_COUNTER["launches"] - n0 == 6 * sum(plan)
        assert torch.isfinite(cached).all() and not torch.equal(cached, plain)
    finally:
        pipe.disable_deepcache()
        pipe.disable_freeu()
