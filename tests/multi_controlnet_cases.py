"""Shared cases of the Multi-ControlNet tests (imd_residual_mix_rows and the mix route): the CPU expression that IS the kernel's contract,
the mistakes a kernel or a host plan could make (each as a variant of that expression), the scale patterns, the crafted values and the
hand-written table.  No GPU is touched on import.

The crafted block.  Two of the mistakes -- the sum taken in another order (K >= 3) and a product contracted with the sum into one fused
multiply-add -- differ from the contract only in the last bit of an fp32 intermediate, which survives the rounding to 16 bits only where
the exact sum lies next to a rounding tie of the element type: about one Gaussian element in 2^12 (fp16) or 2^15 (bf16).  So that no test
depends on that luck, ``crafted_block`` FINDS such elements: it draws 2^20 candidate columns (one 16-bit value per source, Gaussian, seed
fixed) and keeps, for the scales it is given, the first columns at which the variant's 16-bit result differs from the contract's -- the
(x, s) pairs whose product needs more than 24 bits next to an addend that puts the 16-bit result on a tie.  The search is this file's
code, so the block can be re-derived and is never stale; ``test_multi_controlnet_inputs`` asserts that it finds what it is for."""
import torch

from tests.control_rows_cases import DTYPES, bits, host_segments  # noqa: F401  (re-exported for the tests)

MAX_SOURCES = 4
OPEN = (0.7, 1.3, -0.45, 0.9)          # the "all open" scale of source k, the same for every row (the crafted block is found for these)


def _f32(s):
    return torch.tensor(float(s), dtype=torch.float32)


def mix_row(xs, ss, *, order=None, fma=False):
    """the whole contract for one row, on the CPU: ``xs[k]`` 16-bit [n], ``ss[k]`` the scale of source k -> 16-bit [n].
    ``order`` / ``fma``: the two arithmetic mistakes (another order of accumulation; product and sum in float64, rounded once to fp32)."""
    acc = None
    for k in (range(len(xs)) if order is None else order):
        s = float(ss[k])
        if s == 0.0:
            continue                                   # not read, contributes nothing
        if acc is None:
            acc = xs[k].float() * _f32(s)
        elif fma:
            acc = (acc.double() + xs[k].double() * _f32(s).double()).float()
        else:
            acc = acc + xs[k].float() * _f32(s)
    if acc is None:
        return torch.zeros_like(xs[0])
    return acc.to(xs[0].dtype)


def mix(sources, scales, **kw):
    """``sources[k]``: 16-bit [rows, n] on the CPU; ``scales[k][r]`` -> [rows, n]: what the launch leaves in dst"""
    rows = sources[0].shape[0]
    return torch.stack([mix_row([x[r] for x in sources], [sc[r] for sc in scales], **kw) for r in range(rows)])


# ---- the mistakes, as variants of the contract (each must change at least one 16-bit element of the case data) ----
def wrong_dropped(sources, scales):
    return mix(sources[:-1], scales[:-1]) if len(sources) > 1 else torch.zeros_like(sources[0])


def wrong_twice(sources, scales):
    """the last source counted twice (appended once more; for K = 4 it takes the place of nothing: five terms)"""
    rows = sources[0].shape[0]
    return torch.stack([mix_row([x[r] for x in sources] + [sources[-1][r]], [sc[r] for sc in scales] + [scales[-1][r]])
                        for r in range(rows)])


def wrong_transposed(sources, scales):
    """the scales read as [row][k] out of the [k][row] array"""
    K, rows = len(scales), len(scales[0])
    flat = [scales[k][r] for k in range(K) for r in range(rows)]
    return mix(sources, [[flat[r * K + k] for r in range(rows)] for k in range(K)])


def wrong_uncond_neighbour(sources, scales):
    """rows = 2B: uncond row B + j reads the scale of cond row j + 1 instead of j"""
    rows = len(scales[0])
    B = rows // 2
    return mix(sources, [[sc[r] if r < B else sc[(r - B + 1) % B] for r in range(rows)] for sc in scales])


def wrong_order(sources, scales):
    return mix(sources, scales, order=list(reversed(range(len(sources)))))


def wrong_fma(sources, scales):
    return mix(sources, scales, fma=True)


# ---- scale patterns: name -> [K][rows] ----
def scale_patterns(K: int, rows: int):
    """every pattern of the kernel tests for K sources and ``rows`` rows, as (name, scales[k][r])"""
    out = [("open", [[OPEN[k]] * rows for k in range(K)])]
    for z in range(K):
        out.append((f"zero{z}", [[0.0 if k == z else OPEN[k]] * rows for k in range(K)]))
    out.append(("all_zero", [[0.0] * rows for _ in range(K)]))
    for one in range(K):
        out.append((f"one{one}", [[1.0 if k == one else 0.0] * rows for k in range(K)]))
    out.append(("negative", [[-abs(OPEN[k]) - 0.125 * k] * rows for k in range(K)]))
    # a different pattern in every row: row r gates source r % K (K > 1), and every open value depends on (k, r)
    out.append(("per_row", [[0.0 if (K > 1 and r % K == k) else (0.3 + 0.21 * k + 0.17 * r) * (-1.0 if (k + r) % 3 == 0 else 1.0)
                             for r in range(rows)] for k in range(K)]))
    return out


def request_scales(B: int, K: int):
    """[K][2B] as the host plan lays them out: B cond rows with their own values, then the same values for the uncond half"""
    half = [[0.25 + 0.5 * k + 0.125 * j for j in range(B)] for k in range(K)]
    return [h + h for h in half]


# ---- the crafted block ----
CRAFT_CANDIDATES = 1 << 20
CRAFT_KEEP = 8


def crafted_block(dtype, K: int, variant, keep: int = CRAFT_KEEP):
    """-> [K, keep] 16-bit values: the first ``keep`` candidate columns at which ``variant`` (``wrong_order`` / ``wrong_fma``) and the
    contract differ in 16 bits under the OPEN scales.  Fewer than ``keep`` columns (none for a variant that cannot differ at this K) are
    returned as found."""
    g = torch.Generator().manual_seed(20240 + K)
    cand = (torch.randn(K, CRAFT_CANDIDATES, generator=g) * 2.0).to(dtype)
    srcs = [cand[k:k + 1] for k in range(K)]
    sc = [[OPEN[k]] for k in range(K)]
    differs = (bits(variant(srcs, sc)) != bits(mix(srcs, sc)))[0]
    cols = differs.nonzero().flatten()[:keep]
    return cand[:, cols].contiguous()


_special_cache = {}


def specials(dtype, K: int):
    """the values written over the head of every row of source k: [K, m] -- the FMA block, then (K >= 3) the order block"""
    key = (dtype, K)
    if key not in _special_cache:
        blocks = [crafted_block(dtype, K, wrong_fma)] if K >= 2 else []
        if K >= 3:
            blocks.append(crafted_block(dtype, K, wrong_order))
        _special_cache[key] = torch.cat(blocks, dim=1) if blocks else torch.zeros(K, 0, dtype=dtype)
    return _special_cache[key]


def source_buffers(row_elems, rows, dtype, K: int, seed: int = 0):
    """-> per source the ``host_segments`` buffers (sentinels on both sides), Gaussian data from a seed per source with the crafted
    values over the head of every row.  (A segment shorter than the block takes its first values.)"""
    sp = specials(dtype, K)
    return [host_segments(row_elems, rows, dtype, seed=seed + 101 * k, special=sp[k] if sp.shape[1] else None) for k in range(K)]


# ---- the hand-written table: K = 2 nets, R = 3 requests, 10 steps ----
# net 0: one scale for all requests, the window opens late;  net 1: per-request scales and windows, request 2 closes early
TABLE_STEPS = 10
TABLE_ARGS = dict(controlnet_conditioning_scale=[0.5, [1.0, 0.25, 2.0]],
                  control_guidance_start=[0.3, [0.0, 0.2, 0.0]],
                  control_guidance_end=[1.0, [1.0, 1.0, 0.5]])
TABLE_ROWS = (([0.0] * 3 + [0.5] * 7,) * 3,
              ([1.0] * 10, [0.0] * 2 + [0.25] * 8, [2.0] * 5 + [0.0] * 5))
