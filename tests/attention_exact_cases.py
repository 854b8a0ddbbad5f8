"""Integer-valued attention problems whose answer is known to the last place (no GPU import; used by tests/test_attention_exact_gpu.py and,
for the preconditions and the sensitivity of the comparison, by tests/test_attention_exact_inputs.py).

imd_attention takes Q already multiplied by D^-1/2 log2(e) and runs its softmax on exp2.  Handed integer-valued Q and K heads DIRECTLY (no
scale), every score is an integer, every P = 2^(s - m_ref) a power of two that survives the rounding to bf16 / fp16 unchanged, every rescale
2^(m_old - m_new) exact.  With small-integer V the numerator and the denominator are sums of small integers times powers of two in fp32; what
is left inexact is 1 / l, one multiply and the final rounding to 16 bits.  A wrong key set, weight, rescale or mask is many units in the last
place, not noise under a tolerance.

Three families (per head and batch entry different data, so that a head or batch mix-up shows):
  count      Q on one half of the head dims, K on the other, one shared dim that makes every real score the constant c (0 or -8: at -8 a counted
             pad key -- K = 0, score 0 -- weighs 2^8 real keys).  V = 0 / 1 indicators: "every key" (output exactly 1.0), seven single keys (0,
             L-1, L-2, first key of the last 64-key unit, first key of the last 32-key block, 31, 32), D - 8 residue classes j % (D - 8);
             the channel order is rotated per (batch entry, head).
  weighted   Q rows with four entries of +-1, K dense in {-1, 0, 1}, V integer in [-4, 4]: scores within [-4, 4], so that under any reference
             maximum within 8 of the true one (and under fp16's 2^-4 bias of the head-dim-40 variant 13) every P is a NORMAL fp16 number.
  staircase  score = a_i floor(j / 64), a_i from {+9, +3, 0, -3} by query row: +9 passes the deferred maximum's threshold at every 64-key unit
             (reference raised, O rescaled), +3 lets variant 13 grow P unchecked (fp16: overflow, the workgroup runs again as variant 12), -3
             never raises.  K, Q and every reference maximum are integers <= 256.

Expectation: softmax2(S) V in float64; with a second key set round_dt(phase 1) + s2 phase 2 (attention.hip:395-397: the first phase is
rounded to the element type before the add); causal: keys > query masked.

Tolerance (derived, not measured; computed by ``expectation``): |got - want| <= ulp_dt(want) + 2^-20 max|V| for one phase -- the fp32 steps (1 / l, one multiply,
summation of numbers that span more than 24 bits) contribute a few 2^-24 relative, which can only flip the final rounding; the absolute term covers
cancellation in the numerator.  Two phases: the kernel's phase 1 is round_dt(p1 (1 + few 2^-24)), which differs from round_dt(p1) -- by one
ulp_dt(p1) -- only where p1 lies within that fp32 error of a rounding tie; there, and only there, ulp_dt(p1) is added.  (Adding it everywhere
would make the bound blind to a first phase that is not rounded at all: that error is at most ulp_dt(p1) / 2.)  Count family: elements whose
expectation is a multiple of 1 / 2 (the "every key" channel, unseen keys) must EQUAL it (``exact_elements``)."""
import collections
import functools

import torch

F64 = torch.float64
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = (BF16, F16)
DT_NAME = {BF16: "bf16", F16: "f16"}
SIG_BITS = {BF16: 8, F16: 11}              # significand bits, the hidden one included
MIN_EXP = {BF16: -126, F16: -14}           # exponent of the smallest normal number
ABS_TERM = 2.0 ** -20                      # x max|V|

LS = (1, 31, 33, 64, 65, 77, 96, 127, 128, 257, 289)       # L % 64 in {0, 1, 31, 32, 33, 63} (+ the text length 77) at one, two and five 64-key units
L_LONG = 1345                                              # 22 units: the LDS-DMA ring of three wraps seven times; ragged by one key
RESIDUES = (0, 1, 31, 32, 33, 63)


def pad64(n):
    return (n + 63) // 64 * 64


def padded_dims(D):
    """(DPK, DPV) of attention.hip::AttnCfg -- what imd_attn_padded_dims reports (asserted by the GPU file)."""
    return (D + 15) // 16 * 16, (D + 31) // 32 * 32


# form: "generic" | "causal" | "d40" | "staircase";  c: the count family's score;  s2: per batch entry, None = one key set;  split: phase2_rows to try
# (0 = none);  variants: imd_set_tuning(0, .) values to run (() = the shipped default only);  pad_one: k_pad_one settings to run
Case = collections.namedtuple("Case", "name form family D B H N L1 bdiv1 L2 bdiv2 s2 c split variants pad_one")


def _case(form, family, D, B, H, N, L1, bdiv1=1, L2=0, bdiv2=1, s2=None, c=0, split=0, variants=(), pad_one=(False,)):
    fam = family if family != "count" else f"count{c}"
    name = f"{form}-{fam}-D{D}-B{B}H{H}-N{N}-L{L1}" + (f"/{bdiv1}" if bdiv1 > 1 else "") + (f"+L{L2}/{bdiv2}" if L2 else "")
    return Case(name, form, family, D, B, H, N, L1, bdiv1, L2, bdiv2, None if s2 is None else tuple(s2), c, split, tuple(variants), tuple(pad_one))


def is_causal(case):
    return case.form == "causal"


# ---- the problems -----------------------------------------------------------------------------------------------------------------------------
def boundary_key(L):
    """An interior key that starts a 32-key block: the last multiple of 32 in (0, L - 1); None where there is none."""
    j = (L - 2) // 32 * 32
    return j if j > 0 else None


def count_keys(L):
    """The seven single-key channels of the count family (None: the key does not exist at this L)."""
    ks = [0, L - 1, L - 2, (L - 1) // 64 * 64, (L - 1) // 32 * 32, 31, 32]
    return [k if 0 <= k < L else None for k in ks]


def _junk(n_rows, dims, salt):
    """Integers in [-3, 3] that depend on row, dim and salt."""
    i = torch.arange(n_rows, dtype=torch.int64)[:, None]
    d = torch.arange(dims, dtype=torch.int64)[None, :]
    return ((i * 5 + d * 3 + salt) % 7 - 3).to(F64)


def _count_set(case, L, Bk, phase):
    D, H = case.D, case.H
    half = D // 2
    k = torch.zeros(Bk, L, H, D, dtype=F64)
    v = torch.zeros(Bk, L, H, D, dtype=F64)
    j = torch.arange(L)
    cls = D - 8
    for b in range(Bk):
        for h in range(H):
            k[b, :, h, 0] = case.c
            k[b, :, h, half:] = _junk(L, D - half, 11 * b + 3 * h + phase)
            ind = torch.zeros(L, D, dtype=F64)
            ind[:, 0] = 1.0
            for ch, key in enumerate(count_keys(L)):
                if key is not None:
                    ind[key, 1 + ch] = 1.0
            ind[j, 8 + j % cls] = 1.0
            v[b, :, h] = ind.roll(3 * b + 5 * h + phase, dims=1)          # another channel order per (kv batch entry, head, key set)
    return k, v


def _rand(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


def _weighted_set(case, L, Bk, gen):
    D, H = case.D, case.H
    k = _rand(gen, -1, 1, Bk, L, H, D)
    v = _rand(gen, -4, 4, Bk, L, H, D)
    # the keys that the mutations of the host file drop or double sit at score 0 (the median) with V = +-4, so that in EVERY query row their
    # loss moves some channel by more than a unit in the last place (a key at score -4 holds 1 / 16 of that weight)
    sign = (1.0 - 2.0 * (torch.arange(D) % 2)).to(F64) * 4.0
    for key in (L - 1, boundary_key(L)):
        if key is not None:
            k[:, key] = 0.0
            v[:, key] = sign
    return k, v


def _staircase_set(case, L, Bk, gen):
    D, H = case.D, case.H
    half = D // 2
    k = torch.zeros(Bk, L, H, D, dtype=F64)
    k[..., 0] = (torch.arange(L) // 64).to(F64)[None, :, None]
    k[..., half:] = _rand(gen, -3, 3, Bk, L, H, D - half)
    v = _rand(gen, -4, 4, Bk, L, H, D)
    sign = (1.0 - 2.0 * (torch.arange(D) % 2)).to(F64) * 4.0
    for key in (L - 1, boundary_key(L)):
        v[:, key] = sign
    return k, v


STAIR_A = (9.0, 3.0, 0.0, -3.0)


@functools.lru_cache(maxsize=None)
def build(case):
    """dict(q [B, N, H, D], k1 / v1 [B // bdiv1, L1, H, D], k2 / v2 [B // bdiv2, L2, H, D] or None): float64 tensors of integers."""
    D, B, H, N = case.D, case.B, case.H, case.N
    half = D // 2
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)))          # (hash() of a str changes from run to run)
    Bk1 = -(-B // case.bdiv1)
    Bk2 = -(-B // case.bdiv2) if case.L2 else 0
    q = torch.zeros(B, N, H, D, dtype=F64)
    if case.family == "count":
        for b in range(B):
            for h in range(H):
                q[b, :, h, 0] = 1.0
                q[b, :, h, 1:half] = _junk(N, half - 1, 7 * b + 2 * h)
        sets = [_count_set(case, case.L1, Bk1, 0)] + ([_count_set(case, case.L2, Bk2, 1)] if case.L2 else [])
    elif case.family == "weighted":
        pos = torch.rand(B, N, H, D, generator=gen).argsort(-1)[..., :4]
        q.scatter_(-1, pos, _rand(gen, 0, 1, B, N, H, 4) * 2.0 - 1.0)
        sets = [_weighted_set(case, case.L1, Bk1, gen)] + ([_weighted_set(case, case.L2, Bk2, gen)] if case.L2 else [])
    elif case.family == "staircase":
        i = torch.arange(N)
        for b in range(B):
            for h in range(H):
                q[b, :, h, 0] = torch.tensor(STAIR_A, dtype=F64)[(i + b + 2 * h) % 4]
        q[..., 1:half] = _rand(gen, -3, 3, B, N, H, half - 1)
        sets = [_staircase_set(case, case.L1, Bk1, gen)] + ([_staircase_set(case, case.L2, Bk2, gen)] if case.L2 else [])
    else:
        raise ValueError(case.family)
    out = dict(q=q, k1=sets[0][0], v1=sets[0][1], k2=None, v2=None)
    if case.L2:
        out["k2"], out["v2"] = sets[1]
    return out


def vmax(case):
    return 1.0 if case.family == "count" else 4.0


def scores(case, phase=0):
    """Integer scores [B, H, N, L] of key set `phase` (kv batch sharing resolved)."""
    t = build(case)
    k = t["k2" if phase else "k1"]
    bdiv = case.bdiv2 if phase else case.bdiv1
    idx = torch.arange(case.B) // bdiv
    return torch.einsum("bnhd,blhd->bhnl", t["q"], k[idx])


# ---- float64 expectation ------------------------------------------------------------------------------------------------------------------------
def visible(case, L, shift=0):
    """[N, L] bool: the keys a query row may see (causal: key <= query + shift; shift = 0 is the kernel's mask)."""
    if not is_causal(case):
        return torch.ones(case.N, L, dtype=torch.bool)
    return torch.arange(L)[None, :] <= torch.arange(case.N)[:, None] + shift


def softmax2_av(s, v, vis, keyw=None, phantom=0):
    """(softmax2(s) v [B, N, H, D], weights [B, H, N, L]) in float64.  s [B, H, N, L], v [B, L, H, D]; vis [N, L]; keyw [L]: how often each key
    counts (None: once); phantom: that many extra keys with score 0 and V = 0 (pad keys that were not masked)."""
    neg = torch.full_like(s, float("-inf"))
    sm = torch.where(vis, s, neg)
    m = sm.amax(-1, keepdim=True)
    if phantom:
        m = m.clamp_min(0.0)
    w = torch.exp2(sm - m)
    w = torch.where(vis, w, torch.zeros_like(w))            # (a fully masked row: exp2(-inf - -inf) = NaN otherwise; its 0 / 0 below stays)
    if keyw is not None:
        w = w * keyw
    den = w.sum(-1, keepdim=True) + phantom * torch.exp2(-m)
    w = w / den
    return torch.einsum("bhnl,blhd->bnhd", w, v), w


def round_dt(x, dt):
    return x.to(dt).to(F64)


def ulp(x, dt):
    """Spacing of `dt` at the magnitude of x (float64 tensor); the subnormal spacing below the smallest normal number."""
    e = torch.frexp(x.abs())[1] - 1                         # floor(log2 |x|); frexp(0) = (0, 0)
    e = torch.where(x == 0, torch.full_like(e, MIN_EXP[dt]), e).clamp_min(MIN_EXP[dt])
    return torch.exp2((e - (SIG_BITS[dt] - 1)).to(F64))


def near_tie(p1, dt, slack):
    """Does p1 lie within `slack` of a point halfway between two neighbouring `dt` numbers?"""
    r = round_dt(p1, dt)
    return ((p1 - r).abs() - 0.5 * ulp(p1, dt)).abs() <= slack


# want / p1 / tol [B, N, H, D] float64; two [B] bool: a second phase was added; exact [B, N, H, D] bool: elements that must EQUAL want
Expect = collections.namedtuple("Expect", "want p1 two tol dt exact")


def exact_elements(case, want):
    """Count family: where the expectation is a multiple of 1 / 2 -- the "every key" channel (1.0, or 1 + s2 with a second key set), channels whose
    keys the row does not see (0), a lone key (1) -- the kernel's o * (1 / l) is within 2^-23 of a number both element types hold, so the stored
    element EQUALS it: no unit in the last place is granted there.  Returns (mask, want with those elements set to the exact value)."""
    if case.family != "count":
        return torch.zeros_like(want, dtype=torch.bool), want
    snapped = (want * 2.0).round() / 2.0                    # (float64 gives 31 x 1 / 31 = 1 - 1e-16)
    exact = (want - snapped).abs() < 1e-12
    return exact, torch.where(exact, snapped, want)

MUTATIONS = ("phantom", "drop_last", "drop_boundary", "double_boundary", "mask_ge", "mask_gt1", "s2_wrong_batch", "p1_unrounded")


def expectation(case, dt, mutation=None):
    """The float64 expectation of `case` for element type `dt` with its tolerance; `mutation`: the same computed WRONG in one of the ways of
    MUTATIONS (tests/test_attention_exact_inputs.py).  Mutations of the key set apply to the first key set."""
    t = build(case)
    B = case.B
    keyw, phantom, shift = None, 0, 0
    if mutation in ("drop_last", "drop_boundary", "double_boundary"):
        key = case.L1 - 1 if mutation == "drop_last" else boundary_key(case.L1)
        keyw = torch.ones(case.L1, dtype=F64)
        keyw[key] = 2.0 if mutation == "double_boundary" else 0.0
    elif mutation == "phantom":
        phantom = 1
    elif mutation == "mask_ge":
        shift = -1
    elif mutation == "mask_gt1":
        shift = 1
    if shift == 1:          # key N of row N - 1 is a pad key: K = 0 (score 0), V = 0
        s1 = torch.cat([scores(case, 0), torch.zeros(B, case.H, case.N, 1, dtype=F64)], -1)
        v1 = torch.cat([t["v1"], torch.zeros_like(t["v1"][:, :1])], 1)
        vis = torch.arange(case.L1 + 1)[None, :] <= torch.arange(case.N)[:, None] + 1
    else:
        s1, v1, vis = scores(case, 0), t["v1"], visible(case, case.L1, shift)
    idx1 = torch.arange(B) // case.bdiv1
    p1, _ = softmax2_av(s1, v1[idx1], vis, keyw, phantom)
    two = torch.zeros(B, dtype=torch.bool)
    want = p1
    tol = None
    slack = ABS_TERM * vmax(case)
    if case.L2 and case.s2 is not None:
        s2 = torch.tensor(case.s2, dtype=F64)
        if mutation == "s2_wrong_batch":
            s2 = s2.roll(1)
        two = s2 != 0
        idx2 = torch.arange(B) // case.bdiv2
        p2, _ = softmax2_av(scores(case, 1), t["v2"][idx2], visible(case, case.L2))
        first = p1 if mutation == "p1_unrounded" else round_dt(p1, dt)
        sel = two[:, None, None, None]
        want = torch.where(sel, first + s2[:, None, None, None] * p2, p1)
        extra = torch.where(sel & near_tie(p1, dt, slack), ulp(p1, dt), torch.zeros_like(p1))
        tol = ulp(want, dt) + slack + extra
    if tol is None:
        tol = ulp(want, dt) + slack
    exact, want = exact_elements(case, want)
    return Expect(want, p1, two, tol, dt, exact)


def first_phase(case, dt):
    """What out_dup receives: the first phase alone, for every batch entry."""
    e = expectation(case, dt)
    exact, want = exact_elements(case, e.p1)
    return Expect(want, e.p1, torch.zeros(case.B, dtype=torch.bool), ulp(e.p1, dt) + ABS_TERM * vmax(case), dt, exact)


def key_weight(case, key):
    """[B, H, N]: the share of first-set key `key` in every row's softmax (0 where the mask hides it)."""
    idx1 = torch.arange(case.B) // case.bdiv1
    _, w = softmax2_av(scores(case, 0), build(case)["v1"][idx1], visible(case, case.L1))
    return w[..., key]


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------------
def mismatches(got, exp):
    """[B, N, H, D] bool: elements of `got` (anything castable to float64, [B, N, H * D] or [B, N, H, D]) outside the tolerance (NaN / inf count), or
    unequal to the expectation where it is exact."""
    g = got.to(F64).reshape(exp.want.shape)
    return ~((g - exp.want).abs() <= exp.tol) | (exp.exact & (g != exp.want))


def assert_exact(got, exp, what):
    bad = mismatches(got, exp)
    if bool(bad.any()):
        g = got.to(F64).reshape(exp.want.shape)
        b, n, h, d = bad.nonzero()[0].tolist()
        w, x = exp.want[b, n, h, d].item(), g[b, n, h, d].item()
        u = ulp(exp.want[b, n, h, d], exp.dt).item()
        rows = int(bad.any(-1).sum())
        raise AssertionError(f"{what} [{DT_NAME[exp.dt]}]: {int(bad.sum())}/{bad.numel()} elements in {rows} (batch, row, head) rows off; first at batch {b} "
                             f"head {h} query row {n} channel {d}: got {x!r} want {w!r}, {abs(x - w) / u:.2f} ulp apart (tolerance "
                             f"{0.0 if bool(exp.exact[b, n, h, d]) else exp.tol[b, n, h, d].item() / u:.2f} ulp); largest distance {float(((g - exp.want).abs() / ulp(exp.want, exp.dt)).nan_to_num(nan=float('inf')).max()):.2f} ulp")


# ---- the kernel's layouts -------------------------------------------------------------------------------------------------------------------------
def to_heads(x, DP, dt, pad_one=False):
    """[B, L, H, D] -> [B, H, L, DP] zero padded; pad column D = 1 when `pad_one` (imd_attn_params.k_pad_one)."""
    B, L, H, D = x.shape
    out = torch.zeros(B, H, L, DP, dtype=dt)
    out[..., :D] = x.permute(0, 2, 1, 3).to(dt)
    if pad_one and DP > D:
        out[..., D] = 1.0
    return out


def to_heads_t(x, DPV, LP, dt):
    """[B, L, H, D] -> V^T [B, H, DPV, LP], zero padded."""
    B, L, H, D = x.shape
    out = torch.zeros(B, H, DPV, LP, dtype=dt)
    out[:, :, :D, :L] = x.permute(0, 2, 3, 1).to(dt)
    return out


def pack(case, dt, pad_one=False):
    """dict(q, k1, v1t, k2, v2t) in the layouts of attention.hip:13-16 (CPU tensors of `dt`).  Q goes in as it is: no softmax scale."""
    t = build(case)
    dpk, dpv = padded_dims(case.D)
    out = dict(q=to_heads(t["q"], dpk, dt), k1=to_heads(t["k1"], dpk, dt, pad_one), v1t=to_heads_t(t["v1"], dpv, pad64(case.L1), dt), k2=None, v2t=None)
    if case.L2:
        out["k2"] = to_heads(t["k2"], dpk, dt, pad_one)
        out["v2t"] = to_heads_t(t["v2"], dpv, pad64(case.L2), dt)
    return out


# ---- fp32 emulation of the kernels' arithmetic (guards the tolerance derivation) ---------------------------------------------------------------
def emulate(case, dt, thr=8.0, bias=0.0, unchecked=False):
    """The online softmax as the kernels run it, in fp32 on the CPU: 32-key blocks; thr > 0: deferred reference maximum (first block's maximum
    + bias, raised when a score passes it by more than thr -- attention.hip:320-339; unchecked: never raised, attention_d40.hip:965-969, run
    again checked when a denominator leaves fp32) or thr = 0: the exact running maximum (:345-355); P rounded to the element type; numerator and
    denominator accumulated in fp32; o * (1 / l); phase 1 rounded to the element type, w2 * o2 / l2 + phase 1 rounded again.  [B, N, H, D] float64."""
    f32 = torch.float32
    t = build(case)

    def rd(x):
        return x.to(dt).to(f32)

    def phase(ph, chk_thr, unchk):
        L = case.L2 if ph else case.L1
        idx = torch.arange(case.B) // (case.bdiv2 if ph else case.bdiv1)
        q = t["q"].to(f32)
        k = t["k2" if ph else "k1"][idx].to(f32)
        v = t["v2" if ph else "v1"][idx].to(f32)
        vis = visible(case, L)
        B, N, H, D = q.shape
        m = torch.zeros(B, H, N, dtype=f32)
        o = torch.zeros(B, H, N, D, dtype=f32)
        l = torch.zeros(B, H, N, dtype=f32)
        for j0 in range(0, L, 32):
            kb, vb, mk = k[:, j0:j0 + 32], v[:, j0:j0 + 32], vis[:, j0:j0 + 32]
            s = torch.einsum("bnhd,blhd->bhnl", q, kb)
            s = torch.where(mk, s, torch.full_like(s, float("-inf")))
            mx = s.amax(-1)
            if j0 == 0:
                m = rd(mx + bias) if chk_thr > 0 else mx
            else:
                if chk_thr > 0:
                    raise_ = (mx - m > chk_thr) & (not unchk)
                    new = torch.where(raise_, rd(m + (mx - m).clamp_min(0.0)), m)
                else:
                    new = torch.maximum(m, mx)
                alpha = torch.exp2(m - new)
                o = o * alpha[..., None]
                l = l * alpha
                m = new
            p = rd(torch.exp2(s - m[..., None]))
            o = o + torch.einsum("bhnl,blhd->bhnd", p, vb)
            l = l + p.sum(-1)
        return o, l

    def run(unchk):
        o1, l1 = phase(0, thr, unchk)
        ok = bool(torch.isfinite(l1).all())
        first = rd(o1 * (1.0 / l1)[..., None])
        out = first
        if case.L2 and case.s2 is not None:
            o2, l2 = phase(1, thr, unchk)
            ok = ok and bool(torch.isfinite(l2).all())
            s2 = torch.tensor(case.s2, dtype=f32)[:, None, None]
            both = rd(o2 * (s2 / l2)[..., None] + first)
            out = torch.where((s2 != 0)[..., None], both, first)
        return out, ok

    out, ok = run(unchecked)
    if unchecked and not ok:
        out, _ = run(False)
    return out.permute(0, 2, 1, 3).to(F64)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------
S2_BY_B = {2: (1.0, 0.0), 3: (0.5, 0.0, 2.0)}              # powers of two (or 0): s2 * phase 2 stays exact
S2_SPLIT = {2: (1.0, 0.0), 3: (0.5, 2.0, 0.0)}              # phase2_rows = R promises that exactly the rows [0, R) have a second softmax
GENERIC_N = (33, 70, 130, 128)                              # ragged row blocks of the 128-row workgroup and one exact multiple
FAMILIES = (("count", -8), ("count", 0), ("weighted", 0))


def _generic_cases():
    out = []
    for di, D in enumerate((40, 64, 80, 160)):
        for li, L1 in enumerate(LS):
            for fi, (fam, c) in enumerate(FAMILIES):
                n = li + di + fi
                B, H = (2, 3) if (li // 2 + di + fi) % 2 else (3, 2)
                kw = dict(bdiv1=2 if n % 3 == 0 else 1)
                if (li + fi) % 2:                                   # a second key set with its own residue, shared by the whole batch or per entry
                    s2 = S2_BY_B[B] if D == 40 else S2_SPLIT[B]
                    L2 = LS[(li + 4 + di) % len(LS)]
                    if fam == "weighted" and L2 == 1:               # (a one-key second set adds integers up to 4, whose unit in the last place hides a
                        L2 = 31                                     # key lost from the first set; the count family keeps L2 = 1: it adds 0 / 1)
                    kw.update(L2=L2, bdiv2=B if n % 4 < 2 else 1, s2=s2,
                              split=0 if D == 40 else sum(1 for x in s2 if x != 0))
                out.append(_case("generic", fam, D, B, H, GENERIC_N[n % 4], L1, c=c, variants=(3, 4) if D == 40 else (), **kw))       # (3: 64-key blocks, exact maximum; 4 = what N < 512 runs by default)
    return out


def _causal_cases():
    out = []
    for di, D in enumerate((64, 80, 40)):
        for ni, N in enumerate((1, 33, 64, 77, 130)):
            for fi, (fam, c) in enumerate(FAMILIES):
                B, H = (2, 3) if (di + ni + fi) % 2 else (3, 2)
                out.append(_case("causal", fam, D, B, H, N, N, c=c))
    return out


D40_GENERIC_VARIANTS = (1, 2, 3, 4, 5)                      # attention.hip's other template forms (imd_launch_attention, case 40)
D40_PIPELINED_VARIANTS = (6, 7, 8, 9, 10, 11, 12, 13)       # attention_d40.hip
D40_DUP_VARIANTS = (12, 13)                                 # out_dup runs the static-ring kernel in these two forms only


def _d40_cases():
    out = []
    for li, L1 in enumerate(LS + (L_LONG,)):
        for fi, (fam, c) in enumerate((("count", -8), ("weighted", 0))):
            N = 530 if (li + fi) % 2 else 512
            kw = {}
            if li % 2 == fi:                                        # a second key set on one of the two batch rows (the garment rows of a CFG batch)
                kw = dict(L2=LS[(li + 3) % len(LS)] if L1 != L_LONG else 289, bdiv2=2, s2=(1.0, 0.0) if li % 4 < 2 else (0.0, 2.0))
            out.append(_case("d40", fam, 40, 2, 2, N, L1, c=c, variants=D40_GENERIC_VARIANTS + D40_PIPELINED_VARIANTS, pad_one=(True, False), **kw))
    out.append(_case("d40", "count", 40, 2, 3, 530, 96, c=0, L2=33, bdiv2=2, s2=(0.0, 1.0), variants=D40_GENERIC_VARIANTS + D40_PIPELINED_VARIANTS,
                     pad_one=(True, False)))
    return out


def _staircase_cases():
    return [_case("staircase", "staircase", 40, 2, 2, 130, 640),
            _case("staircase", "staircase", 80, 2, 2, 130, 640),
            _case("staircase", "staircase", 40, 2, 2, 512, 640, variants=(12, 13), pad_one=(True, False))]


GENERIC_CASES = _generic_cases()
CAUSAL_CASES = _causal_cases()
D40_CASES = _d40_cases()
STAIRCASE_CASES = _staircase_cases()
ALL_CASES = GENERIC_CASES + CAUSAL_CASES + D40_CASES + STAIRCASE_CASES


def case_id(case):
    return case.name
