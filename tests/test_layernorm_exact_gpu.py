"""LayerNorm to the last place at every site that normalises token rows (inputs, float64 expectation, bars, mutants: tests/layernorm_cases.py;
that the bars are met by a correct fp32 kernel and by no mutant: tests/test_layernorm_inputs.py).

  S1  norm.hip::layernorm_kernel (one wave per row, C <= 2048)                        ops.layer_norm, general affine and unit affine
  S2  row_common.h::ln_rows_inplace (lanes l / l ^ 32 share a row) in row_linear.hip  ops.linear(x, eye(320), ln_eps=eps)            tile config 12
  S3  the same function in row_qkv.hip                                                weight [I; I; I], head-split Q / K / V^T      tile config 15
  S4  written out in row_linear_k640.hip (two waves exchange partial sums in LDS)     eye(640), row-major and head-split Q          tile config 13
  S5  row_linear_k1280.hip (four-way exchange, two row halves)                        eye(1280), row-major and head-split Q         tile config 14
  S6  a further copy in ff_fused.hip                                                  ops.ff_geglu_fused with selector weights

The fused sites are reached with an identity weight: the normalised row is rounded to the element type before the MFMA and is exact through
it, so the launch returns round_dt(n) and the bar is the element bar of layernorm_cases on n64 itself.  Every family (general, large_mean,
eps_dominated at both eps, constant, outlier) and both element types at every site; on ``general`` also the scale statistic, which is what sees
a variance divided by K - 1 in bf16.  M takes the row-block edges of each kernel (128 rows; 64 for K = 1280; four rows per block in S1).

row_xattn.hip is NOT isolated here: its softmax sits between the LayerNorm and any output.  It calls ln_rows_inplace, the function S2 and S3
pin, and keeps its parity test (tests/test_text_xattn_gpu.py).

Each check prints its worst element error in ulp and, on ``general``, its |s - 1| (pytest -rA)."""
import pytest
import torch

from tests import exact_cases as ec
from tests import layernorm_cases as lc

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTS = pytest.mark.parametrize("dt", lc.DTYPES, ids=[lc.DT_NAME[d] for d in lc.DTYPES])
ROW_MS = (1, 127, 128, 129, 300)           # 128-row blocks (row_linear.hip, row_linear_k640.hip, ff_fused.hip)
K1280_MS = (1, 63, 64, 65, 200)            # 64-row blocks, two 16-token halves per wave


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def dev(t, dt=None):
    return (t if dt is None else t.to(dt)).to("cuda")


def host(t):
    return t.to(F64).cpu()


_EYES = {}


def eye(K, dt, copies=1):
    key = (K, dt, copies)
    if key not in _EYES:
        _EYES[key] = torch.eye(K, dtype=dt, device="cuda").repeat(copies, 1).contiguous()
    return _EYES[key]


def check(got, y, dt, A, what, ulp=None, scale=None):
    """The element bar on every element; ``scale`` = (K, rows): also the scale statistic over the first ``rows`` rows."""
    assert tuple(got.shape) == tuple(y.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(y.shape)}"
    ok, worst, of_bar, bad = lc.element_bar(got, y, dt, A, ulp)
    line = f"{what}: worst element error {worst:.3f} ulp, {of_bar:.3f} of the bar"
    s_err = None
    if scale is not None:
        K, rows = scale
        s_err = abs(lc.scale_statistic(got[:rows], y[:rows]) - 1.0)
        line += f", |s - 1| = {s_err:.3g} (bound {lc.scale_bound(K, dt, rows):.3g})"
    print(line)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert ok, f"{what}: {bad} of {got.numel()} elements beyond ulp + A (worst {worst:.3f} ulp)"
    if s_err is not None:
        assert s_err <= lc.scale_bound(K, dt, rows), f"{what}: |s - 1| = {s_err:.3g} > {lc.scale_bound(K, dt, rows):.3g}"


def scale_key(case, K, M):
    return (K, M) if case.family == "general" and M in lc.SCALE_ROWS[K] else None


# ---- S1 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 4, 5, 77])
@pytest.mark.parametrize("C", lc.S1_CS)
@DTS
def test_layer_norm(ops, C, rows, dt):
    """norm.hip::layernorm_kernel with a general affine (element bar on y = n64 gamma + beta) and, on ``general``, with the unit affine (scale statistic)."""
    gamma, beta = ec.away_from_zero_affine(11, C)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    for case in lc.family_cases(C, dt):
        sub = case._replace(x=lc.take_rows(case.x, rows))
        x = dev(sub.x, dt)
        y, A = lc.affine_expectation(sub, gamma, beta)
        check(host(ops.layer_norm(x, dev(gamma), dev(beta), case.eps)), y, dt, A, f"layer_norm C={C} rows={rows} {case.name}")
        if case.family == "general":
            check(host(ops.layer_norm(x, one, zero, case.eps)), lc.reference(sub.x, case.eps), dt, lc.abs_term(case),
                  f"layer_norm C={C} rows={rows} {case.name}, unit affine", scale=scale_key(case, C, rows))


@pytest.mark.parametrize("C", [2056, 2052])
@DTS
def test_layer_norm_refuses_what_it_cannot_hold(ops, C, dt):
    x = torch.zeros(4, C, dtype=dt, device="cuda")
    with pytest.raises(ops.L.ImdError):
        ops.layer_norm(x, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"))


# ---- S2, S4, S5: LayerNorm -> identity projection, row-major ------------------------------------------------------------------------------------
def ln_identity(ops, x64, K, eps, dt):
    """round_dt(n) of the rows x64 [M, K] from the row-resident projection of width K (the C ABI picks the kernel by K)."""
    return ops.linear(dev(x64, dt), eye(K, dt), torch.zeros(K, device="cuda"), ln_eps=eps)


def run_row_major(ops, K, M, dt, name):
    for case in lc.family_cases(K, dt):
        x = lc.take_rows(case.x, M)
        got = ln_identity(ops, x, K, case.eps, dt)
        assert got.dtype == dt
        check(host(got), lc.reference(x, case.eps), dt, lc.abs_term(case), f"{name} M={M} {case.name}", scale=scale_key(case, K, M))


@pytest.mark.parametrize("M", ROW_MS)
@DTS
def test_row_linear_k320(ops, M, dt):
    run_row_major(ops, 320, M, dt, "row_linear.hip (cfg 12)")


@pytest.mark.parametrize("M", ROW_MS)
@DTS
def test_row_linear_k640(ops, M, dt):
    run_row_major(ops, 640, M, dt, "row_linear_k640.hip (cfg 13)")


@pytest.mark.parametrize("M", K1280_MS)
@DTS
def test_row_linear_k1280(ops, M, dt):
    run_row_major(ops, 1280, M, dt, "row_linear_k1280.hip (cfg 14)")


# ---- head-split epilogues -----------------------------------------------------------------------------------------------------------------------
def unsplit(q, B, HW, D):
    """[B, H, HW, DP] -> [B HW, H D]"""
    return q[..., :D].permute(0, 2, 1, 3).reshape(B * HW, -1)


def same_where_normal(a, b, dt, scale, what):
    """a = (value stored with ``scale``) / scale against b: a power-of-two scale is exact, except that the scaled value may be subnormal in fp16."""
    floor = 0.0 if dt == torch.bfloat16 else 2.0 ** -14 / scale
    differ = (a != b) & (b.abs() >= floor)
    assert not bool(differ.any()), f"{what}: {int(differ.sum())} elements differ"


@pytest.mark.parametrize("K,B,HW,D", [(640, 2, 150, 80), (1280, 2, 100, 160)], ids=["k640", "k1280"])
@DTS
def test_head_split_q(ops, K, B, HW, D, dt):
    """S4 / S5 once through the head-split Q epilogue (8 heads, scale 0.25): the same rows as the row-major launch, and the bar."""
    H, scale = 8, 0.25
    DPK, _ = ops.attn_padded_dims(D)
    M = B * HW
    sub = 0.0 if dt == torch.bfloat16 else 2.0 ** -24 / scale            # fp16: a scaled value below 2^-14 is stored on the subnormal grid
    for case in lc.family_cases(K, dt):
        x = lc.take_rows(case.x, M)
        q = torch.zeros(B, H, HW, DPK, dtype=dt, device="cuda")
        ops.conv_gemm(dev(x, dt), eye(K, dt), M=M, N=K, Cin=K, Hin=HW, Win=1, Hout=HW, Wout=1, bias=torch.zeros(K, device="cuda"), ln_eps=case.eps,
                      heads=dict(C=K, H=H, D=D, dests=[(q, 0, DPK, HW, scale)]))
        got = host(unsplit(q, B, HW, D)) / scale
        what = f"head-split Q K={K} {case.name}"
        check(got, lc.reference(x, case.eps), dt, lc.abs_term(case) + sub, what, scale=scale_key(case, K, M))
        same_where_normal(got, host(ln_identity(ops, x, K, case.eps, dt)), dt, scale, what + " vs row-major")
        assert float(q[..., D:].abs().max()) == 0.0 if DPK > D else True


# ---- S3 -----------------------------------------------------------------------------------------------------------------------------------------
@DTS
def test_row_qkv(ops, dt):
    """row_qkv.hip with the weight [I; I; I]: Q / 0.5, K and V^T transposed are ONE tensor, equal to what row_linear.hip returns for the same rows
    (both call ln_rows_inplace), and meet the bar; pad columns (Q, K: dims 40 .. 47) and pad rows (V^T: 40 .. 63) stay zero."""
    B, HW, K, H, D = 3, 128, 320, 8, 40
    DPK, DPV = ops.attn_padded_dims(D)
    LP = ops.pad64(HW)
    M = B * HW
    sub = 0.0 if dt == torch.bfloat16 else 2.0 ** -24 / 0.5
    for case in lc.family_cases(K, dt):
        x = lc.take_rows(case.x, M)
        q, k = (torch.zeros(B, H, HW, DPK, dtype=dt, device="cuda") for _ in range(2))
        vt = torch.zeros(B, H, DPV, LP, dtype=dt, device="cuda")
        ops.conv_gemm(dev(x, dt), eye(K, dt, 3), M=M, N=3 * K, Cin=K, Hin=HW, Win=1, Hout=HW, Wout=1, bias=torch.zeros(3 * K, device="cuda"), ln_eps=case.eps,
                      heads=dict(C=K, H=H, D=D, dests=[(q, 0, DPK, HW, 0.5), (k, 0, DPK, HW, 1.0), (vt, 1, DPV, LP, 1.0)]))
        gq, gk = host(unsplit(q, B, HW, D)) / 0.5, host(unsplit(k, B, HW, D))
        gv = host(vt[:, :, :D, :HW].permute(0, 3, 1, 2).reshape(M, K))
        y = lc.reference(x, case.eps)
        what = f"row_qkv.hip (cfg 15) {case.name}"
        check(gk, y, dt, lc.abs_term(case), what + " K", scale=(K, 300) if case.family == "general" else None)
        check(gv, y, dt, lc.abs_term(case), what + " V^T")
        check(gq, y, dt, lc.abs_term(case) + sub, what + " Q")
        assert torch.equal(gk, gv), f"{what}: K and V^T differ"
        same_where_normal(gq, gk, dt, 0.5, what + " Q / 0.5 vs K")
        assert torch.equal(gk, host(ln_identity(ops, x, K, case.eps, dt))), f"{what}: differs from row_linear.hip on the same rows"
        assert float(q[..., D:].abs().max()) == 0.0 and float(k[..., D:].abs().max()) == 0.0 and float(vt[:, :, D:].abs().max()) == 0.0
        assert float(vt[..., HW:].abs().max()) == 0.0 if LP > HW else True


# ---- S6 -----------------------------------------------------------------------------------------------------------------------------------------
_FF = {}


def ff_selector(ops, dt):
    """Weights that make the feed-forward return x + LN(x): value rows j < 320 of w1 are e_j, the gate is the constant 8 (gelu_erf_f(8) == 8 in fp32:
    its exp2 term is 1e-14), w2[i, j] = delta_ij / 8."""
    if dt not in _FF:
        Cc, inner = 320, 1280
        w1 = torch.zeros(2 * inner, Cc)
        w1[:Cc] = torch.eye(Cc)
        b1 = torch.cat([torch.zeros(inner), torch.full((inner,), 8.0)])
        w2 = torch.zeros(Cc, inner)
        w2[:, :Cc] = torch.eye(Cc) / 8
        _FF[dt] = ops.pack_ff_fused(dev(w1, dt), dev(b1), dev(w2, dt), dev(torch.zeros(Cc)), dev(torch.ones(Cc)), dev(torch.zeros(Cc)))
        assert _FF[dt]["ln"]
    return _FF[dt]


@pytest.mark.parametrize("M", ROW_MS)
@DTS
def test_ff_geglu_fused(ops, M, dt):
    """ff_fused.hip's copy of the LayerNorm.  Its header: "h is rounded to the 16-bit element type before the second GEMM (as the GEGLU tensor was
    when it went through memory), fp32 accumulation everywhere"; the normalised row is packed to the element type in front of the first GEMM and the
    residual is added to the fp32 accumulator.  With the selector weights h = 8 round_dt(n) exactly, the second GEMM returns round_dt(n) exactly,
    and the launch stores round_dt(x + round_dt(n)).  Bar: ulp_dt(n64) + ulp_dt(x + n64) / 2 + A (layernorm_cases.ff_expectation)."""
    packed = ff_selector(ops, dt)
    for case in lc.family_cases(320, dt):
        x = lc.take_rows(case.x, M)
        want, ulp = lc.ff_expectation(case, M, dt)
        got = host(ops.ff_geglu_fused(dev(x, dt), packed, case.eps))
        what = f"ff_fused.hip M={M} {case.name}"
        check(got, want, dt, lc.abs_term(case), what, ulp=ulp)
        if case.family == "general" and M == lc.GENERAL_ROWS:
            s_err, bound = lc.ff_scale(got, dt)
            print(f"{what}: |s - 1| = {s_err:.3g} over the rows scaled by 2^-6 .. 2^-4 (bound {bound:.3g})")
            assert s_err <= bound, f"{what}: |s - 1| = {s_err:.3g} > {bound:.3g}"
