"""GroupNorm statistics from every producer and through every fold, on integer-valued data where the answer is known EXACTLY
(tests/exact_cases.py; preconditions and the sensitivity of the comparison: tests/test_gn_exact_inputs.py).

Producers -- the statistics pass, the concatenation that writes statistics on the way, the halo-patch epilogues, the finish launch of K-sliced
convolutions, the register-staged tiles: the stored tensor EQUALS the float64 reference cast to the element type, and the fp32 partials, folded in
float64, EQUAL the exact (sum, sum of squares) of every (image, group).  No tolerance: one element dropped, counted twice or credited to the
neighbouring group fails.

Consumers -- gn_apply_kernel (unrolled and loop fold), gn_coeffs_kernel (+ gn_apply_coeffs_kernel on large maps), gemm_common.h::gn_in_coeffs: fed
partials crafted here (integer pieces, negative ones and zeros among them, that sum to the exact statistics), so no producer is involved.  With exact
S and Q and var >= mean^2 the fp32 chain S / n, Q / n - mean^2, rsqrtf, one multiply carries a relative error of about 2e-6: coefficient a within
1e-5 relative, b within 1e-5 (|beta| + |mean a|), the 16-bit output within one unit in the last place at the reference's magnitude, every element.

Large mean -- the folds use E[x^2] - mean^2 in fp32: rstd within 1e-3 of float64 up to |mean| / std = 32 (r^2 2^-23 times a small summation factor
is about 1e-4); |mean| / std = 128 (fp16) is measured only (profiles/gn_large_mean_error.txt)."""
import pytest
import torch

from tests import exact_cases as ec

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTS = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def dev(t, dt=None):
    return (t if dt is None else t.to(dt)).to("cuda")


def pack_conv(w):  # [Cout, Cin, kh, kw] -> [Cout, kh*kw*Cin]
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def check_producer(stored, want, part, nparts, G, dt, what):
    """The three assertions of a producer case: the stored tensor, the folded partials, the partials' shape."""
    B = want.shape[0]
    assert stored.dtype == dt and tuple(stored.shape) == tuple(want.shape), f"{what}: stored {tuple(stored.shape)} {stored.dtype}"
    bad = stored.cpu() != want.to(dt)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} stored elements differ from the exact reference, first at {bad.nonzero()[0].tolist()}"
    assert part.dtype == torch.float32 and tuple(part.shape) == (B, nparts, G, 2), f"{what}: partials {tuple(part.shape)}, the library reports {nparts} parts"
    exact, _ = ec.group_sums(want, G)
    if not ec.partials_match(part, exact):
        got = part.to(F64).sum(1).cpu()
        b, g, k = (got != exact).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((got != exact).sum())} of {exact.numel()} folded statistics differ from the exact sums; first at image {b} group {g} "
                             f"({'S' if k == 0 else 'Q'}): got {got[b, g, k].item():.1f}, exact {exact[b, g, k].item():.1f}")


def pass_partials(ops, x, G):
    """Run the statistics pass on x [B, HW, C] (through group_norm_coeffs) and read its partials back from the shared workspace."""
    B, HW, C = x.shape
    assert getattr(x, "_imd_gn_stats", None) is None
    ab = ops.group_norm_coeffs(x, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), groups=G, eps=EPS)
    lib = ops.L.load()
    nws = lib.imd_groupnorm_workspace_floats(B, HW, C, G)
    part = ops.workspace("gn_partial", (max(nws, 1),), torch.float32, x.device)
    nchunks = lib.imd_groupnorm_parts(B, HW, C)
    assert nchunks == ec.gn_chunks(B, HW, C), "tests/exact_cases.py's copy of norm.hip's chunking is out of date"
    assert nchunks * B * G * 2 + 2 * B * C == nws
    return part[: B * nchunks * G * 2].view(B, nchunks, G, 2).clone(), nchunks, ab


# ---- producers ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.STATS_PASS_CASES + [ec.two_level_case()], ids=str)
@DTS
def test_statistics_pass(ops, case, dt):
    B, HW, C, G = case
    want = ec.plain_tensor(1, B, HW, C, G)
    x = dev(want, dt)
    part, nchunks, _ = pass_partials(ops, x, G)
    check_producer(x, want, part, nchunks, G, dt, f"gn_stats_kernel {case}")


@pytest.mark.parametrize("case,rounding", [(c, False) for c in ec.CONCAT_CASES] + [(c, True) for c in ec.CONCAT_CASES if c[7]],
                         ids=lambda v: str(v) if isinstance(v, tuple) else ("rounded-sums" if v else "exact-sums"))
@DTS
def test_concatenation_with_statistics(ops, case, rounding, dt):
    B, H, W, Ca, Cb, G, half, ctrl = case
    a, b, add, want = ec.concat_operands(2, *case, dt, rounding=rounding)
    out = ops.concat_channels(dev(a, dt), dev(b, dt), None if add is None else dev(add, dt), gn_stats_groups=G)
    st = getattr(out, "_imd_gn_stats", None)
    assert st is not None and st[2] == G, "the concatenation must hand its statistics on"
    assert st[1] == ops.L.load().imd_groupnorm_parts(B, H * W, Ca + Cb)
    check_producer(out, want, st[0], st[1], G, dt, f"concat2_stats_kernel {case}")


def run_conv(ops, d, dt, Cout, **kw):
    return ops.conv2d_nhwc(dev(d["x"], dt), dev(pack_conv(d["w"]), dt), dev(d["bias"].float()), rowvec=dev(d["temb"].float()), rowvec_stride=Cout,
                           res=dev(d["res"], dt), stride=d["stride"], taps=d["taps"], ups=d["ups"], **kw)


@pytest.mark.parametrize("case", ec.PATCH_CASES, ids=str)
@DTS
def test_halo_patch_epilogue_statistics(ops, case, dt):
    cfg, B, H, W, Cin, Cout, G, ups = case
    d = ec.patch_conv(case)
    out = run_conv(ops, d, dt, Cout, cfg=cfg, split_k=1, gn_stats_groups=G)
    st = getattr(out, "_imd_gn_stats", None)
    assert st is not None and st[2] == G, f"tile config {cfg} must hand its statistics on"
    check_producer(out, d["out"], st[0], st[1], G, dt, f"halo-patch epilogue {case}")


@pytest.mark.parametrize("case", ec.SPLITK_CASES, ids=str)
@DTS
def test_splitk_finish_statistics(ops, case, dt):
    cfg, B, H, W, Cin, Cout, G, split, stride = case
    d = ec.splitk_conv(case)
    out = run_conv(ops, d, dt, Cout, cfg=cfg, split_k=split, gn_stats_groups=G)
    st = getattr(out, "_imd_gn_stats", None)
    assert st is not None and st[2] == G, "the finish launch must hand its statistics on"
    check_producer(out, d["out"], st[0], st[1], G, dt, f"split-K finish {case}")


@pytest.mark.parametrize("case", ec.TILE_CASES, ids=str)
@DTS
def test_register_staged_tile_statistics(ops, monkeypatch, case, dt):
    cfg, B, H, W, Cin, Cout, G, stride, taps, T = case
    monkeypatch.setattr(ops, "GENERIC_GN_STATS", True)
    d = ec.tile_conv(case)
    out = run_conv(ops, d, dt, Cout, cfg=cfg, split_k=1, gn_stats_groups=G)
    st = getattr(out, "_imd_gn_stats", None)
    assert st is not None and st[2] == G, f"tile config {cfg} must hand its statistics on"
    check_producer(out, d["out"], st[0], st[1], G, dt, f"register-staged tiles {case}")


# ---- consumers ----------------------------------------------------------------------------------------------------------------------------------
def general_affine(C):
    g = torch.Generator().manual_seed(6)
    return (1.0 + 0.3 * torch.randn(C, generator=g)).float(), (0.5 * torch.randn(C, generator=g)).float()


def check_coeffs(a, b, ref, beta, what):
    a, b = a.to(F64).cpu(), b.to(F64).cpu()
    rel = ((a - ref["a"]).abs() / ref["a"].abs()).max().item()
    slack = ((b - ref["b"]).abs() / (beta.to(F64).abs() + ref["mean_a"].abs())).max().item()
    print(f"{what}: a rel err {rel:.3g}, b err / (|beta| + |mean a|) {slack:.3g}")
    assert rel <= 1e-5, f"{what}: coefficient a off by {rel:.3g} relative"
    assert slack <= 1e-5, f"{what}: coefficient b off by {slack:.3g} (|beta| + |mean a|)"


def check_output(y, ref_y, dt, what):
    assert y.dtype == dt
    err = (y.to(F64).cpu() - ref_y).abs() / ec.ulp_at(ref_y, dt)
    print(f"{what}: max error {err.max().item():.3f} ulp")
    assert bool((err <= 1.0).all()), f"{what}: {int((err > 1.0).sum())} of {err.numel()} elements beyond one ulp (max {err.max().item():.3f})"


@pytest.mark.parametrize("k", range(5), ids=["one", "two", "unrolled-limit", "limit+1", "cap"])
@pytest.mark.parametrize("G", ec.CONSUMER_GROUPS)
@DTS
def test_folds_of_crafted_partials(ops, G, k, dt):
    """gn_coeffs_kernel and gn_apply_kernel on partials no producer wrote."""
    assert ops.FUSED_GN_STATS
    nparts = ec.consumer_nparts(G)[k]
    B, HW, C = ec.consumer_shape(G)
    x64 = ec.plain_tensor(3, B, HW, C, G)
    sums, _ = ec.group_sums(x64, G)
    pieces = ec.split_partials(5 + k, sums, nparts)
    x = dev(x64, dt)
    x._imd_gn_stats = (dev(pieces.float()), nparts, G)
    gamma, beta = general_affine(C)
    a, b = ops.group_norm_coeffs(x, dev(gamma), dev(beta), groups=G, eps=EPS)
    check_coeffs(a, b, ec.gn_reference(x64, G, gamma, beta, EPS), beta, f"gn_coeffs_kernel G={G} nparts={nparts}")
    g2, b2 = ec.away_from_zero_affine(7, C)
    for silu in (False, True):
        y = ops.group_norm(x, dev(g2), dev(b2), groups=G, eps=EPS, silu=silu)
        check_output(y, ec.gn_reference(x64, G, g2, b2, EPS, silu)["y"], dt, f"gn_apply_kernel ({ec.consumer_branch('apply', G, nparts)}) G={G} nparts={nparts} silu={silu}")
    # the folds really read the partials they were handed: other statistics, other coefficients
    wrong = pieces.clone()
    wrong[:, nparts - 1, :, 1] += sums[..., 1]
    x._imd_gn_stats = (dev(wrong.float()), nparts, G)
    a2, _ = ops.group_norm_coeffs(x, dev(gamma), dev(beta), groups=G, eps=EPS)
    assert float(((a2 - a).abs() / a.abs()).min()) > 0.1


def _gn_in_cases():
    out = []
    for cfg, K, HW in ec.GN_IN_KERNELS:
        for G in ec.GN_IN_GROUPS[K]:
            for k in (range(5) if K == 320 else (2, 3)):
                out.append((cfg, K, HW, G, k))
    return out


@pytest.mark.parametrize("cfg,K,HW,G,k", _gn_in_cases())
@pytest.mark.parametrize("silu", [False, True])
@DTS
def test_fold_inside_the_row_resident_projections(ops, monkeypatch, cfg, K, HW, G, k, silu, dt):
    """gemm_common.h::gn_in_coeffs: the projection's weight is the identity, so the launch returns the normalised rows (rounded to the element type
    before the MFMA, exact through it)."""
    assert ops.FUSED_GN_STATS and ops.FUSED_GN_PROJ and cfg in ops.FUSED_GN_PROJ_CFGS
    nparts = ec.consumer_nparts(G)[k]
    B = 2
    x64 = ec.plain_tensor(4, B, HW, K, G)
    sums, _ = ec.group_sums(x64, G)
    x = dev(x64, dt).view(B, HW // 8, 8, K)
    x._imd_gn_stats = (dev(ec.split_partials(9 + k, sums, nparts).float()), nparts, G)
    gamma, beta = ec.away_from_zero_affine(8, K)

    def no_second_launch(*a, **kw):
        raise AssertionError("the projection fell back to a separate group_norm launch")
    monkeypatch.setattr(ops, "group_norm", no_second_launch)
    eye = torch.eye(K, dtype=dt, device="cuda")
    y = ops.conv2d_nhwc(x, eye, torch.zeros(K, device="cuda"), taps=1, cfg=cfg, gn_in=(dev(gamma), dev(beta), EPS, silu, G))
    check_output(y.view(B, HW, K), ec.gn_reference(x64, G, gamma, beta, EPS, silu)["y"], dt,
                 f"gn_in_coeffs ({ec.consumer_branch('gn_in', G, nparts)}) cfg={cfg} G={G} nparts={nparts} silu={silu}")


@DTS
def test_two_level_fold_of_an_ordinary_call(ops, dt):
    """More than 256 chunks: gn_stats_kernel -> gn_coeffs_kernel -> gn_apply_coeffs_kernel."""
    B, HW, C, G = ec.two_level_case()
    assert ops.L.load().imd_groupnorm_parts(B, HW, C) == ec.GN_TWO_LEVEL_CHUNKS + 1
    assert ops.L.load().imd_groupnorm_parts(B, HW - 1, C) == ec.GN_TWO_LEVEL_CHUNKS
    x64 = ec.plain_tensor(1, B, HW, C, G)
    x = dev(x64, dt)
    gamma, beta = general_affine(C)
    a, b = ops.group_norm_coeffs(x, dev(gamma), dev(beta), groups=G, eps=EPS)
    check_coeffs(a, b, ec.gn_reference(x64, G, gamma, beta, EPS), beta, "group_norm_coeffs, 257 chunks")
    g2, b2 = ec.away_from_zero_affine(7, C)
    for silu in (False, True):
        y = ops.group_norm(x, dev(g2), dev(b2), groups=G, eps=EPS, silu=silu)
        check_output(y, ec.gn_reference(x64, G, g2, b2, EPS, silu)["y"], dt, f"group_norm, 257 chunks, silu={silu}")


# ---- large mean ---------------------------------------------------------------------------------------------------------------------------------
LARGE_MEAN_R = {torch.bfloat16: (1, 8, 32), torch.float16: (1, 8, 32, 128)}      # (bf16 cannot hold std 1 at mean 128: its spacing there is 1)


def large_mean_error(ops, dt, r):
    """Max relative error of rstd (fp32 fold of the statistics pass vs float64 on the same 16-bit tensor) at |mean| / std = r, std 1; the mean's sign
    alternates from group to group.  [2, 256, 320], 32 groups: 2560 elements per (image, group)."""
    B, HW, C, G = 2, 256, 320, 32
    g = torch.Generator().manual_seed(100 + r)
    sign = (1.0 - 2.0 * (torch.arange(G) % 2)).repeat_interleave(C // G)
    x = (torch.randn(B, HW, C, generator=g) + r * sign).to(dt)
    ref = ec.gn_reference(x.to(F64), G, torch.ones(C), torch.zeros(C), EPS)
    assert float((ref["mean"].abs() * ref["rstd"] / r - 1).abs().max()) < 0.1      # the data has the |mean| / std it claims
    a, _ = ops.group_norm_coeffs(dev(x), torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), groups=G, eps=EPS)
    return ((a.to(F64).cpu() - ref["a"]).abs() / ref["a"]).max().item()


@pytest.mark.parametrize("dt,r", [(dt, r) for dt, rs in LARGE_MEAN_R.items() for r in rs], ids=lambda v: str(v).replace("torch.", ""))
def test_large_mean(ops, r, dt):
    err = large_mean_error(ops, dt, r)
    print(f"|mean| / std = {r}, {dt}: rstd relative error {err:.3g}")
    if r <= 32:
        assert err <= 1e-3, f"rstd off by {err:.3g} relative at |mean| / std = {r}"
