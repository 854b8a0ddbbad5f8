"""Inputs, float64 expectations, bars, fp32 emulations and mutants for the LayerNorm tests (tests/test_layernorm_inputs.py on the host,
tests/test_layernorm_exact_gpu.py on the GPU).  CPU only: torch on the host, nothing of the package is imported here.

Every site computes  n = (x - mean) / sqrt(var + eps)  of a token row of K channels with the BIASED variance, in fp32, two passes, and rounds once
to the 16-bit element type.  Rows are [rows, K], seeded, rounded to the element type first; the reference is float64 on those rounded values.

Families (``family_cases``):
  general        randn 1.5 plus a per-channel offset 0.6 randn; row i is multiplied by 2^(i % 13 - 6) (LayerNorm is scale-invariant away from eps,
                 neighbouring rows differ by a factor of two).  300 rows: the scale statistic below is quiet.
  large_mean     randn + r with alternating sign per row, r in {8, 32} (bf16) / {8, 32, 128} (fp16: bf16's spacing at 128 is 1, it cannot hold std 1 there).
                 bf16 has one more member, r = 388 on bf16's own grid (LARGE_MEAN_CENTRE): the only regime in which a 16-bit bar can see a one-pass
                 variance at K = 320 / 640 in bf16.
  eps_dominated  every element is +-2^-9, half of each sign, signs permuted per row: mean exactly 0, variance exactly 2^-18 = 3.8e-6, in both element
                 types and in fp32.  Run at eps 1e-5 and 1e-6 (the two values the models use): |n| = 2^-9 / sqrt(2^-18 + eps) = 0.526 / 0.891.
  constant       rows of c in {0, 1.5, -96}: n = 0.
  outlier        unit noise with one channel at 200 (row i: channel K - 1 - 7 i), |n| there about sqrt(K).

Element bar:  |got - y| <= ulp_dt(y) + A.  Half an ulp is the final rounding; the fp32 steps in front of it (a few 2^-24 relative) can only flip it:
the emulation of a correct kernel stays at about half an ulp on ``general``.  A covers elements near zero, where an ulp means nothing:
  general, eps_dominated, outlier   A = 2^-20 (the attention suite's absolute term);
  large_mean     A = 2 x the largest pre-rounding absolute error of a plain fp32 two-pass LayerNorm with strictly sequential sums over the case
                 (``emulate``; both output forms the kernels use: (x - mean) rstd, and fma(x, rstd, -mean rstd) whose shift is rounded at magnitude r).
                 Measured against that emulation, never a kernel; stored per (K, dtype, r) in LARGE_MEAN_A, checked by the host test;
  constant       |c| 2^-22 / sqrt(eps): mean = sum (1 / K) carries two roundings (2^-23 |c| relative to c), the fused form's shift one more; x - mean is
                 then that residue and rstd = 1 / sqrt(eps).  Every value must be finite.
With an affine (S1) A is multiplied by |gamma| of the channel and a cancellation term is added (``affine_expectation``); the feed-forward site
(S6) returns x + n, rounded a second time (``ff_expectation``, ``ff_scale``).

Scale statistic, on ``general`` without affine:  s = <got, y> / <y, y>  over the case.  A variance divided by K - 1 moves every output by 1 / (2 K) =
0.04 .. 0.16 % -- below half a bf16 ulp, invisible to the element bar, but |s - 1| = 1 / (2 K).  The bound on |s - 1| is
``scale_bound`` = 4 x the value of the ideal kernel round_dt(y), stored per (K, dtype, rows) in SCALE_IDEAL (the host test recomputes it).  The ideal
value is the rounding's own bias (2e-7 .. 8e-5 here); a correct fp32 kernel differs from the ideal one only where its noise flips a rounding and
lands within a few per cent of it, the smallest scale error of interest, 1 / (2 x 2048), is 2.4e-4.

Mutants (``MUTANTS``): float64 restatements of wrong kernels (the one-pass variance in fp32: its fault is an fp32 one).  Which regime catches which:
see MUTANT_CAUGHT_BY; tests/test_layernorm_inputs.py asserts it for K in {320, 640, 1280} and both types."""
import collections
import functools

import torch

from tests import exact_cases as ec

F64 = torch.float64
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = (BF16, F16)
DT_NAME = {BF16: "bf16", F16: "f16"}
KS = (320, 640, 1280)                                           # the row-resident kernels
S1_CS = (8, 320, 512, 520, 768, 1024, 1280, 2048)               # ops.layer_norm: 512 = one vector per lane, 520 = a second vector on one lane, 2048 = the limit
ALL_C = tuple(sorted(set(KS) | set(S1_CS)))
EPS_VALUES = (1e-5, 1e-6)
A_ABS = 2.0 ** -20
GENERAL_ROWS = 300
LARGE_MEAN_R = {BF16: (8, 32, 388), F16: (8, 32, 128)}
# bf16 only: randn + 448.  bf16's spacing there is 2, so the rounded noise has std sqrt(1 + 4 / 12) = 1.155 and |mean| / std = 388 -- the largest
# ratio eight significant bits hold with a spread of about one spacing.  A one-pass variance in fp32 is off by 2 mean^2 2^-24 .. 2^-23 = 1 .. 4 % of
# that variance, rstd by half of it: more than the bf16 ulp (0.4 .. 0.8 %).  At r = 32 its error is 1e-4 and no 16-bit bar can see it.
LARGE_MEAN_CENTRE = {388: 448.0}
CONSTANTS = (0.0, 1.5, -96.0)
# rows of ``general`` over which the scale statistic is taken (a prefix of the case): what each GPU site runs at its largest M
SCALE_ROWS = {C: ((77,) if C in S1_CS else ()) + ({320: (300,), 640: (300,), 1280: (200,)}.get(C, ())) for C in ALL_C}

Case = collections.namedtuple("Case", "name family x eps A")      # x [rows, K] float64, exact in the element type; A: float, or None = the constant bound


def round_dt(t: torch.Tensor, dt) -> torch.Tensor:
    return t.to(dt).to(F64)


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _dtk(dt) -> int:
    return 1 if dt == BF16 else 2


# ---- families -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general(K: int, dt) -> torch.Tensor:
    g = _gen(1, K, _dtk(dt))
    x = torch.randn(GENERAL_ROWS, K, generator=g, dtype=F64) * 1.5 + 0.6 * torch.randn(1, K, generator=g, dtype=F64)
    j = torch.arange(GENERAL_ROWS) % 13 - 6
    return round_dt(x * torch.ldexp(torch.ones(GENERAL_ROWS, dtype=F64), j)[:, None], dt)


@functools.lru_cache(maxsize=None)
def large_mean(K: int, dt, r: int) -> torch.Tensor:
    g = _gen(2, K, _dtk(dt), r)
    sign = 1.0 - 2.0 * (torch.arange(64) % 2).to(F64)
    return round_dt(torch.randn(64, K, generator=g, dtype=F64) + LARGE_MEAN_CENTRE.get(r, float(r)) * sign[:, None], dt)


@functools.lru_cache(maxsize=None)
def eps_dominated(K: int) -> torch.Tensor:
    g = _gen(3, K)
    base = torch.cat([torch.full((K // 2,), 2.0 ** -9, dtype=F64), torch.full((K - K // 2,), -(2.0 ** -9), dtype=F64)])
    return torch.stack([base[torch.randperm(K, generator=g)] for _ in range(16)])


def constant(K: int, c: float) -> torch.Tensor:
    return torch.full((5, K), c, dtype=F64)


@functools.lru_cache(maxsize=None)
def outlier(K: int, dt) -> torch.Tensor:
    g = _gen(4, K, _dtk(dt))
    x = torch.randn(16, K, generator=g, dtype=F64)
    for i in range(16):
        x[i, (K - 1 - 7 * i) % K] = 200.0
    return round_dt(x, dt)


def constant_bound(c: float, eps: float) -> float:
    return abs(c) * 2.0 ** -22 / eps ** 0.5


@functools.lru_cache(maxsize=None)
def family_cases(K: int, dt):
    """Every case of (K, dtype), ``general`` first.  Treat the tensors as read-only."""
    out = [Case("general", "general", general(K, dt), 1e-5, A_ABS)]
    out += [Case(f"large_mean r={r}", "large_mean", large_mean(K, dt, r), 1e-5, LARGE_MEAN_A[(K, DT_NAME[dt], r)]) for r in LARGE_MEAN_R[dt]]
    out += [Case(f"eps_dominated eps={e:g}", "eps_dominated", eps_dominated(K), e, A_ABS) for e in EPS_VALUES]
    out += [Case(f"constant c={c:g} eps={e:g}", "constant", constant(K, c), e, None) for c in CONSTANTS for e in EPS_VALUES]
    out += [Case("outlier", "outlier", outlier(K, dt), 1e-5, A_ABS)]
    return tuple(out)


def take_rows(x: torch.Tensor, M: int) -> torch.Tensor:
    """The first M rows of a case, the case repeated where it is shorter."""
    reps = (M + x.shape[0] - 1) // x.shape[0]
    return (x if reps == 1 else x.repeat(reps, 1))[:M].contiguous()


# ---- expectation and bars -----------------------------------------------------------------------------------------------------------------------
def reference(x: torch.Tensor, eps: float) -> torch.Tensor:
    """n64: float64 LayerNorm without affine, biased variance."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)


def abs_term(case: Case) -> float:
    if case.A is not None:
        return case.A
    return constant_bound(float(case.x[0, 0]), case.eps)


def element_bar(got: torch.Tensor, y: torch.Tensor, dt, A, ulp=None):
    """-> (ok, worst |got - y| in units of ``ulp`` over the elements whose ulp exceeds 4 A -- elsewhere an ulp means nothing --, worst |got - y| as a
    fraction of the bar ``ulp + A``, elements beyond the bar).  ``A``: float or per-element tensor; ``ulp``: per-element tensor, default ulp_dt(y)."""
    got = got.to(F64)
    ulp = ec.ulp_at(y, dt) if ulp is None else ulp
    err = (got - y).abs()
    bar = ulp + A
    finite = bool(torch.isfinite(got).all())
    bad = ~(err <= bar)                                          # (NaN compares false: counted)
    in_ulp = torch.where(ulp > 4 * A, err / ulp, torch.zeros_like(err)).nan_to_num(nan=float("inf"))
    of_bar = (err / bar).nan_to_num(nan=float("inf"))
    return finite and not bool(bad.any()), float(in_ulp.max()), float(of_bar.max()), int(bad.sum())


def affine_expectation(case: Case, gamma: torch.Tensor, beta: torch.Tensor):
    """S1 -> (y = n64 gamma + beta, per-element absolute term).  gamma / beta: exact_cases.away_from_zero_affine (|beta| about 5).  Unlike the integer
    data that affine was made for, |n| here exceeds 3, so n gamma and beta CAN cancel: ulp(y) vanishes there while the fp32 error of the two terms
    stays.  n carries the chain's relative error (mean, deviations and their 1 / K, rsqrt at one ulp, the multiply: four roundings, 2^-22), beta's
    add one more rounding at the larger magnitude: 2^-22 (|n gamma| + |beta|), about 2.6e-6 where they cancel and far below an ulp everywhere else."""
    n = reference(case.x, case.eps)
    g, b = gamma.to(F64), beta.to(F64)
    y = n * g + b
    return y, g.abs() * abs_term(case) + 2.0 ** -22 * ((n * g).abs() + b.abs())


def ff_expectation(case: Case, M: int, dt):
    """S6 -> (want = x + n64, the bar's ulp term = ulp_dt(n64) + half an ulp of the sum).  The launch returns round_dt(x + round_dt(n)):
    round_dt(n) is within the element bar of n64, the sum is rounded once more: half an ulp at the sum's magnitude.  That sum is x + round_dt(n),
    up to ulp(n64) away from x + n64 and possibly in the next binade: the half ulp is taken at |x + n64| + ulp(n64)."""
    x = take_rows(case.x, M)
    n = reference(x, case.eps)
    return x + n, ec.ulp_at(n, dt) + ec.ulp_at((x + n).abs() + ec.ulp_at(n, dt), dt) / 2


def scale_statistic(got: torch.Tensor, y: torch.Tensor) -> float:
    return float((got.to(F64) * y).sum() / (y * y).sum())


def scale_ideal(K: int, dt, rows: int) -> float:
    y = reference(general(K, dt)[:rows], 1e-5)
    return abs(scale_statistic(round_dt(y, dt), y) - 1.0)


def scale_bound(K: int, dt, rows: int) -> float:
    return 4.0 * SCALE_IDEAL[(K, DT_NAME[dt], rows)]


def _ff_rows():
    """S6 returns x + n rounded once more: at the large scales of ``general`` that rounding (an ulp of |x|) buries n.  Its scale statistic is taken
    over the rows scaled by 2^-6 .. 2^-4 (|x| < 0.5 or so), as  <got - x, n64> / <n64, n64>."""
    return (torch.arange(GENERAL_ROWS) % 13) <= 2


def ff_scale_ideal(dt) -> float:
    x = general(320, dt)[_ff_rows()]
    n = reference(x, 1e-5)
    return abs(scale_statistic(round_dt(x + round_dt(n, dt), dt) - x, n) - 1.0)


def ff_scale(got: torch.Tensor, dt):
    """got [300, 320]: the launch's output for general(320, dtype) -> (|s - 1|, its bound = 4 x the ideal round_dt(x + round_dt(n64)))."""
    x = general(320, dt)[_ff_rows()]
    return abs(scale_statistic(got.to(F64)[_ff_rows()] - x, reference(x, 1e-5)) - 1.0), 4.0 * FF_SCALE_IDEAL[DT_NAME[dt]]


# ---- fp32 emulation of a correct kernel ---------------------------------------------------------------------------------------------------------
def _seq_sum32(cols) -> torch.Tensor:
    s = torch.zeros_like(cols[0])
    for c in cols:
        s = s + c
    return s


def emulate(x: torch.Tensor, eps: float, form: str = "fused") -> torch.Tensor:
    """Plain fp32 two-pass LayerNorm with strictly sequential sums -> the value BEFORE the rounding to the element type, as float64.
    form "fused": mean = sum (1 / K), squared deviations by fma, n = fma(x, rstd, -mean rstd) (row_common.h::ln_rows_inplace and its copies);
    form "div":   mean = sum / K, n = (x - mean) rstd (norm.hip::layernorm_kernel).  fma(a, b, c) is taken as float32(float64(a) float64(b) + c): the
    product is exact in float64.  rsqrt is the correctly rounded one."""
    K = x.shape[-1]
    x32 = x.to(torch.float32)
    f32 = torch.float32
    inv_k = torch.tensor(1.0, dtype=f32) / torch.tensor(float(K), dtype=f32)
    s = _seq_sum32(x32.unbind(-1))
    mean = s * inv_k if form == "fused" else s / float(K)
    d = x32 - mean[:, None]
    if form == "fused":
        sq = torch.zeros_like(s)
        for c in d.unbind(-1):
            sq = (c.to(F64) * c.to(F64) + sq.to(F64)).to(f32)
        var = sq * inv_k
    else:
        var = _seq_sum32((d * d).unbind(-1)) / float(K)
    rstd = (1.0 / torch.sqrt((var + torch.tensor(eps, dtype=f32)).to(F64))).to(f32)
    if form == "fused":
        shift = -mean * rstd
        n = (x32.to(F64) * rstd.to(F64)[:, None] + shift.to(F64)[:, None]).to(f32)
    else:
        n = d * rstd[:, None]
    return n.to(F64)


FORMS = ("fused", "div")


def large_mean_a(K: int, dt, r: int) -> float:
    x = large_mean(K, dt, r)
    y = reference(x, 1e-5)
    return 2.0 * max(float((emulate(x, 1e-5, f) - y).abs().max()) for f in FORMS)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------
def _norm(x, mean, var, eps):
    return (x - mean) / torch.sqrt(var + eps)


def _m_eps_swapped(x, eps):
    return reference(x, 1e-6 if eps == 1e-5 else 1e-5)


def _m_eps_zero(x, eps):
    return reference(x, 0.0)


def _m_var_k_minus_1(x, eps):
    K = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    return _norm(x, mean, ((x - mean) ** 2).sum(-1, keepdim=True) / (K - 1), eps)


def _m_mean_first_half(x, eps):
    K = x.shape[-1]
    mean = x[:, : K // 2].mean(-1, keepdim=True)
    return _norm(x, mean, ((x - mean) ** 2).mean(-1, keepdim=True), eps)


def _m_sqdev_second_half_dropped(x, eps):
    K = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    return _norm(x, mean, ((x - mean)[:, : K // 2] ** 2).sum(-1, keepdim=True) / K, eps)


def _m_one_pass_fp32(x, eps):
    """var = E[x^2] - mean^2 in fp32, sequential sums, times 1 / K as the kernels write it."""
    K = x.shape[-1]
    f32 = torch.float32
    x32 = x.to(f32)
    inv_k = torch.tensor(1.0, dtype=f32) / torch.tensor(float(K), dtype=f32)
    mean = _seq_sum32(x32.unbind(-1)) * inv_k
    var = _seq_sum32((x32 * x32).unbind(-1)) * inv_k - mean * mean
    rstd = (1.0 / torch.sqrt((var + torch.tensor(eps, dtype=f32)).to(F64))).to(f32)
    return ((x32 - mean[:, None]) * rstd[:, None]).to(F64)


def _m_channel_left_out(x, eps):
    K = x.shape[-1]
    mean = x[:, : K - 1].sum(-1, keepdim=True) / K
    return _norm(x, mean, ((x - mean)[:, : K - 1] ** 2).sum(-1, keepdim=True) / K, eps)


def _m_rstd_of_neighbour(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(torch.roll(var, 1, 0) + eps)


MUTANTS = {
    "eps swapped": _m_eps_swapped,
    "eps = 0": _m_eps_zero,
    "variance / (K - 1)": _m_var_k_minus_1,
    "mean of the first half": _m_mean_first_half,
    "squared deviations of the second half dropped": _m_sqdev_second_half_dropped,
    "one-pass variance in fp32": _m_one_pass_fp32,
    "one channel left out of both sums": _m_channel_left_out,
    "rstd of the neighbouring row": _m_rstd_of_neighbour,
}


# The checks that MUST reject each mutant at every K and in both types (others may reject it as well):
#   a wrong or missing eps shows only where the variance is of eps' size; at variance 2 it changes the seventh digit;
#   K - 1 is a pure scale error of 1 / (2 K): under half a bf16 ulp for every element, so only the statistic over the whole case sees it in bf16;
#   a mean over half the row misses the per-channel offsets of ``general`` (0.6 / sqrt(K / 2) of a std: many ulps);
#   half the squared deviations: every output times sqrt(2);
#   one-pass: its error is mean^2 2^-23 relative to the variance -- r = 128 in fp16, bf16's own grid at r = 388 (see LARGE_MEAN_CENTRE);
#   a channel left out: the outlier family puts its 200 on the last channel of row 0; at r = 32 the mean moves by 32 / K;
#   the neighbour's rstd: neighbouring rows of ``general`` differ by a factor of two.
MUTANT_CAUGHT_BY = {
    "eps swapped": {BF16: ("eps_dominated eps=1e-05", "eps_dominated eps=1e-06"), F16: ("eps_dominated eps=1e-05", "eps_dominated eps=1e-06")},
    "eps = 0": {BF16: ("eps_dominated eps=1e-05", "eps_dominated eps=1e-06"), F16: ("eps_dominated eps=1e-05", "eps_dominated eps=1e-06")},
    "variance / (K - 1)": {BF16: ("scale statistic",), F16: ("scale statistic",)},
    "mean of the first half": {BF16: ("general",), F16: ("general",)},
    "squared deviations of the second half dropped": {BF16: ("general", "eps_dominated eps=1e-05"), F16: ("general", "eps_dominated eps=1e-05")},
    "one-pass variance in fp32": {BF16: ("large_mean r=388",), F16: ("large_mean r=128",)},
    "one channel left out of both sums": {BF16: ("outlier", "large_mean r=32"), F16: ("outlier", "large_mean r=32")},
    "rstd of the neighbouring row": {BF16: ("general",), F16: ("general",)},
}


def run_checks(fn, K: int, dt, scale_rows=None):
    """Apply ``fn(x, eps) -> pre-rounding n`` (an emulation or a mutant) to every case of (K, dtype), round to the element type, and run every check
    the GPU module runs -> the names of the checks that FAIL ("general", "large_mean r=32", ..., "scale statistic")."""
    failed = []
    for case in family_cases(K, dt):
        y = reference(case.x, case.eps)
        got = round_dt(fn(case.x, case.eps), dt)
        ok, _, _, _ = element_bar(got, y, dt, abs_term(case))
        if not ok:
            failed.append(case.name)
        if case.family == "general":
            for rows in (scale_rows or SCALE_ROWS.get(K, ())):
                if abs(scale_statistic(got[:rows], y[:rows]) - 1.0) > scale_bound(K, dt, rows):
                    failed.append("scale statistic")
                    break
    return failed


# ---- stored constants (tests/test_layernorm_inputs.py recomputes every one from the functions above) ---------------------------------------------
# 2 x the largest pre-rounding |emulate - float64| over large_mean(K, dtype, r), both output forms: large_mean_a
LARGE_MEAN_A = {
    (8, "bf16", 8): 1.2141821894573468e-06, (8, "bf16", 32): 3.894715514096703e-06, (8, "bf16", 388): 6.0463322250736695e-05, (8, "f16", 8): 1.6255664472275555e-06, (8, "f16", 32): 5.163648423955891e-06, (8, "f16", 128): 2.0125187412123324e-05,
    (320, "bf16", 8): 1.3445595609340444e-05, (320, "bf16", 32): 1.3096906709364475e-05, (320, "bf16", 388): 6.88834287214668e-05, (320, "f16", 8): 1.031433212972388e-05, (320, "f16", 32): 1.4228832542428904e-05, (320, "f16", 128): 2.4109882996725673e-05,
    (512, "bf16", 8): 2.801543924846328e-05, (512, "bf16", 32): 3.0575624534456836e-05, (512, "bf16", 388): 5.401920600345278e-05, (512, "f16", 8): 3.4669041477641827e-06, (512, "f16", 32): 2.0532231437719872e-05, (512, "f16", 128): 3.032133591673869e-05,
    (520, "bf16", 8): 3.7778923092091077e-06, (520, "bf16", 32): 2.32082343138984e-05, (520, "bf16", 388): 6.229788612044374e-05, (520, "f16", 8): 3.7050219363621295e-06, (520, "f16", 32): 2.425879442125023e-05, (520, "f16", 128): 2.5246035153969615e-05,
    (640, "bf16", 8): 2.812067550639341e-05, (640, "bf16", 32): 2.887078827296108e-05, (640, "bf16", 388): 7.188129552915257e-05, (640, "f16", 8): 7.891623772238177e-06, (640, "f16", 32): 1.1708005654753606e-05, (640, "f16", 128): 2.997046434494166e-05,
    (768, "bf16", 8): 3.791217965698479e-05, (768, "bf16", 32): 3.4007842894645535e-05, (768, "bf16", 388): 8.947188399588413e-05, (768, "f16", 8): 2.622067164903541e-05, (768, "f16", 32): 1.006945353587696e-05, (768, "f16", 128): 4.0572534620864076e-05,
    (1024, "bf16", 8): 3.6414781861005e-05, (1024, "bf16", 32): 5.206310647221102e-05, (1024, "bf16", 388): 6.631157752590155e-05, (1024, "f16", 8): 3.8296025319795035e-06, (1024, "f16", 32): 4.5460228766280864e-05, (1024, "f16", 128): 4.155544285566748e-05,
    (1280, "bf16", 8): 2.26284326787507e-05, (1280, "bf16", 32): 6.271246514977236e-05, (1280, "bf16", 388): 8.907083142428718e-05, (1280, "f16", 8): 1.9159299706750232e-05, (1280, "f16", 32): 1.728930197852918e-05, (1280, "f16", 128): 4.581900191791277e-05,
    (2048, "bf16", 8): 3.8389678152839224e-05, (2048, "bf16", 32): 9.28093522691853e-05, (2048, "bf16", 388): 0.00013196024545969465, (2048, "f16", 8): 6.1315878179257766e-06, (2048, "f16", 32): 2.022395616751993e-05, (2048, "f16", 128): 0.0001023031622295889,
}

# |s - 1| of the ideal kernel round_dt(y) over the first ``rows`` rows of general(K, dtype): scale_ideal
SCALE_IDEAL = {
    (8, "bf16", 77): 7.64749240333984e-05, (8, "f16", 77): 4.780578935381641e-06,
    (320, "bf16", 77): 8.089608240613444e-06, (320, "bf16", 300): 5.556276225782142e-06, (320, "f16", 77): 1.7516758182845038e-06, (320, "f16", 300): 2.856325145961236e-06,
    (512, "bf16", 77): 9.825472250035716e-06, (512, "f16", 77): 4.204321857326221e-07,
    (520, "bf16", 77): 1.6181475644971854e-05, (520, "f16", 77): 3.5056376325171e-06,
    (640, "bf16", 300): 8.017750231625875e-06, (640, "f16", 300): 3.3948856348331446e-07,
    (768, "bf16", 77): 7.490125635500888e-06, (768, "f16", 77): 1.5198270022498406e-06,
    (1024, "bf16", 77): 1.4138687699061236e-05, (1024, "f16", 77): 1.2914372722327983e-06,
    (1280, "bf16", 77): 9.655373321204586e-06, (1280, "bf16", 200): 7.471715955720271e-06, (1280, "f16", 77): 1.8510372992164292e-06, (1280, "f16", 200): 2.1355279291590534e-06,
    (2048, "bf16", 77): 1.4217964432905461e-05, (2048, "f16", 77): 2.0201927153351562e-07,
}

# |s - 1| of the ideal feed-forward site round_dt(x + round_dt(n64)) over the small-scale rows of general(320, dtype): ff_scale_ideal
FF_SCALE_IDEAL = {"bf16": 6.620975928972594e-05, "f16": 2.8250916361827194e-07}
