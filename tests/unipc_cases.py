"""Shared by the fused-UniPC tests (TEST INFRASTRUCTURE, no test in here): the float64 statement of ``imd_unipc_step``, the operands and
coefficient blocks of the EXACT family with the check of its preconditions, the derived parity bound, and the oracle that starts at a
later schedule position."""
import torch

from oracle.unipc import UniPCOracle

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


class StartOracle(UniPCOracle):
    """oracle/unipc.py for a run that begins at ``timesteps[start]`` (inpainting ``strength`` < 1): ``set_timesteps`` leaves the step
    index where diffusers' ``_init_step_index`` would put it -- the caller slices ``timesteps`` itself (oracle.pipeline.denoise)"""

    def __init__(self, start=0, **kw):
        super().__init__(**kw)
        self.start = int(start)

    def set_timesteps(self, n):
        ts = super().set_timesteps(n)
        self.step_index = self.start
        return ts


def step_ref(z, eps, g_rows, c, H, blend=None, absolute=False):
    """float64 statement of ``imd_unipc_step`` for one block c (``ops.unipc_coefs`` order).  z [B,HW,4], eps [2B,HW,4], g_rows [B],
    H [K,B,HW,4] by physical slot (not modified), blend = (mask [B,HW], z_img, blend_noise) -> dict(e, m, s, z_un, z, parts) with
    ``parts`` every intermediate in evaluation order.  ``absolute``: the same expression on the absolute values of every coefficient
    and operand -- the quantity A of the parity bound."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    f = (lambda v: abs(float(v))) if absolute else float
    B = z.shape[0]
    z, cc, uu = ab(z.double()), ab(eps[:B].double()), ab(eps[B:].double())
    gr = ab(g_rows.double().view(B, 1, 1))
    parts = []

    def keep(t):
        parts.append(t)
        return t
    d = keep(cc + uu if absolute else cc - uu)
    e = keep(uu + keep(gr * d))
    m = keep(keep(f(c[0]) * z) + keep(f(c[1]) * e))
    s = keep(keep(f(c[2]) * z) + keep(f(c[3]) * m))
    for k in range(H.shape[0]):
        s = keep(s + keep(f(c[4 + k]) * ab(H[k].double())))
    zn = keep(keep(f(c[8]) * s) + keep(f(c[9]) * m))
    for k in range(H.shape[0]):
        zn = keep(zn + keep(f(c[10 + k]) * ab(H[k].double())))
    z_un = zn
    if blend is not None:
        mask, z_img, bn = (ab(t.double()) for t in blend)
        mk = mask.unsqueeze(-1)
        proper = keep(keep(f(c[14]) * z_img) + keep(f(c[15]) * bn))
        one_m = keep(1.0 + mk if absolute else 1.0 - mk)
        zn = keep(keep(one_m * proper) + keep(mk * zn))
    x = keep(f(c[16]) * zn)
    return dict(e=e, m=m, s=s, z_un=z_un, z=zn, x=x, parts=parts)


# ---- the exact family: every operand in {-2, 0, 2}, masks in {0, 1} and {0.5}, integer guidance, coefficients in
# {0, +-1/4, +-1/2, +-1, 2}: every intermediate is a small dyadic rational, every sum exact in fp32 whatever the contraction ----
EXACT_VALUES = (-2.0, 0.0, 2.0)
EXACT_COEFS = (0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0)
EXACT_SHAPES = [(B, HW) for B in (1, 3) for HW in (1, 63, 64, 257)]          # the grid's tail, and a row boundary inside a wavefront
EXACT_K = (0, 2, 4)


def _pick(values, seed, *shape):
    idx = torch.randint(0, len(values), shape, generator=torch.Generator().manual_seed(seed))
    return torch.tensor(values, dtype=torch.float32)[idx]


def exact_operands(B, HW, K):
    """-> dict of CPU fp32 tensors: z, eps, H [K,...], z_img, bn, mask01, mask05, g_rows (integers)"""
    return dict(z=_pick(EXACT_VALUES, 1, B, HW, 4), eps=_pick(EXACT_VALUES, 2, 2 * B, HW, 4), H=_pick(EXACT_VALUES, 3, K, B, HW, 4),
                z_img=_pick(EXACT_VALUES, 4, B, HW, 4), bn=_pick(EXACT_VALUES, 5, B, HW, 4), mask01=_pick((0.0, 1.0), 6, B, HW),
                mask05=torch.full((B, HW), 0.5), g_rows=torch.tensor([3.0, 7.0, 5.0][:B]))


def exact_blocks(K):
    """[(name, the 19 values)]: three general blocks with every coefficient from the set, and the indicator blocks -- exactly one
    coefficient of a group non-zero, so that a swapped s_h / z_h entry, or store_m / store_s, fails by name"""
    from imagdressing_amd import ops
    pairs = [(-1, -1)] if K == 0 else [(0, 1), (1, 0), (K - 1, -1), (-1, K - 1), (K - 1, 0)]
    sm, ss = pairs[0]
    out = []
    for n in range(3):
        v = _pick(EXACT_COEFS, 40 + n, 17).tolist()
        a, b = pairs[n % len(pairs)]
        out.append((f"general{n}", ops.unipc_coefs(v[0], v[1], v[2], v[3], v[4:4 + K], v[8], v[9], v[10:10 + K], v[14], v[15],
                                                   (0.5, 0.25, 2.0)[n], a, b)))
    base = dict(m_x=1.0, m_e=-0.5, s_x=0.0, s_m=0.0, z_s=0.0, z_m=0.0, b_img=0.5, b_noise=-0.25, in_scale=0.5, store_m=sm, store_s=ss)
    for name in ("m_x", "m_e"):                              # m alone, seen through s_m = 1 (s' = m) and the store of m
        out.append((f"only {name}", ops.unipc_coefs(**{**base, "m_x": 0.0, "m_e": 0.0, "s_m": 1.0, name: 2.0})))
    for name in ("s_x", "s_m"):                              # the corrector's terms one at a time (z' = 0: z_s = 0)
        out.append((f"only {name}", ops.unipc_coefs(**dict(base, **{name: 2.0}))))
    for k in range(K):
        out.append((f"only s_h[{k}]", ops.unipc_coefs(**dict(base, s_h=[2.0 if j == k else 0.0 for j in range(K)]))))
    for name in ("z_s", "z_m"):                              # the predictor's terms one at a time, from s' = z
        out.append((f"only {name}", ops.unipc_coefs(**dict(base, s_x=1.0, **{name: -0.5}))))
    for k in range(K):
        out.append((f"only z_h[{k}]", ops.unipc_coefs(**dict(base, s_x=1.0, z_h=[-0.5 if j == k else 0.0 for j in range(K)]))))
    for a, b in pairs[1:]:                                   # every store pattern: m != s' here, so a swap shows
        out.append((f"stores {a},{b}", ops.unipc_coefs(**dict(base, s_x=1.0, s_m=0.25, z_s=1.0, z_m=0.5, store_m=a, store_s=b))))
    return out


def is_exact_fp32(t):
    return bool(torch.equal(t.float().double(), t))


# ---- the parity bound ----
PARITY_ROUNDINGS = 32          # the chain e -> m -> s' -> z' -> blend is at most 24 rounded operations deep; contraction only removes some


def parity_bound(z, eps, g_rows, c, H, blend=None):
    """-> dict(m, s, z, x): 32 * 2^-24 * A elementwise, A = ``step_ref`` on the absolute values"""
    A = step_ref(z, eps, g_rows, c, H, blend, absolute=True)
    u = PARITY_ROUNDINGS * 2.0 ** -24
    return dict(m=u * A["m"], s=u * A["s"], z=u * A["z"], x=u * A["x"])


def half_ulp(ref, dtype):
    """half a unit in the last place of ``dtype`` (fp16 / bf16) at the float64 values ``ref``"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    ex = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - mant)
