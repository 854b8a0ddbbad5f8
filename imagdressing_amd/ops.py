"""Typed wrappers around the C ABI that take torch tensors as *device memory handles* only
(``data_ptr()`` + the current HIP stream).  No torch math happens here; CPU tensors, wrong dtypes
and non-contiguous views raise -- there is no eager fallback.
"""
from __future__ import annotations

import functools
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib as L

ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2, 3, 4
bf16 = torch.bfloat16
f16 = torch.float16
DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1}     # IMD_DTYPE_*


def _code(t: torch.Tensor, name: str = "tensor") -> int:
    """Element-type code of a 16-bit activation/weight tensor (bf16 or fp16; both run the MFMA at the
    same rate, fp16 is what the reference computes in)."""
    try:
        return DTYPE_CODE[t.dtype]
    except KeyError:
        raise L.ImdError(f"{name}: expected a bfloat16 or float16 tensor, got {t.dtype}") from None


try:        # the raw handle of torch's current stream without building a torch.cuda.Stream object per call (6 x ~4 us per processor call)
    _raw_stream, _cur_dev = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
except AttributeError:      # (a torch build without the private entry points)
    _raw_stream = _cur_dev = None


def _stream() -> int:
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype, name: str) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise L.ImdError(f"{name}: tensor is on {t.device}; imagdressing_amd runs on MI355X only (no CPU path)")
    if t.dtype != dtype:
        raise L.ImdError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.ImdError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], dtype, name: str) -> Optional[int]:
    return None if t is None else _dev(t, dtype, name)


_checked_devices = set()


def ensure_device(device: torch.device):
    if device.type != "cuda":
        raise L.ImdError(f"tensor is on {device}; imagdressing_amd runs on MI355X (gfx950) only -- there is no CPU path")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _checked_devices:
        L.check(L.load().imd_device_check(idx))
        _checked_devices.add(idx)


# ---------------------------------------------------------------------------------------------
# persistent zero-initialised workspaces (attention Q/K/V^T buffers rely on their padding staying 0)
# ---------------------------------------------------------------------------------------------
_ws: Dict[Tuple, torch.Tensor] = {}


def workspace(tag: str, shape: Sequence[int], dtype, device, init=None) -> torch.Tensor:
    """Persistent scratch keyed by (tag, shape, dtype, device, CURRENT STREAM): launches on one stream are ordered, so one buffer
    per stream is race-free; two pipelines driven on two streams of one process get separate buffers instead of silently sharing."""
    key = (tag, tuple(shape), dtype, device.type, device.index, _stream()) if isinstance(device, torch.device) else (tag, tuple(shape), dtype, str(device), None, _stream())
    t = _ws.get(key)
    if t is None:
        t = torch.zeros(tuple(shape), dtype=dtype, device=device)
        if init is not None:
            init(t)
        _ws[key] = t
    return t


def k_buffer(shape: Sequence[int], D: int, dtype, device, tag: Optional[str] = None) -> torch.Tensor:
    """Zeroed K operand [Bk, H, L, DPK] of the attention kernels.  When the head dim leaves pad columns (D = 40 -> DPK = 48)
    column D is set to 1.0 ONCE: it is the slot through which the deferred row maximum enters the QK^T MFMA
    (``imd_attn_params.k_pad_one``).  The projection epilogue writes columns [0, D) only, so the 1 persists."""
    def init(t):
        if t.shape[-1] > D:
            t[..., D] = 1.0
    if tag is not None:
        return workspace(tag, shape, dtype, device, init=init)
    t = torch.zeros(tuple(shape), dtype=dtype, device=device)
    init(t)
    return t


def clear_workspaces(stream: Optional[int] = None):
    """Drop every persistent scratch buffer (attention operand buffers, GroupNorm partials, split-K slabs, cached fp8 K / V).
    ``stream`` (a raw stream handle, ``torch.cuda.Stream.cuda_stream``): only the buffers keyed by THAT stream -- what a pipeline calls
    when it releases its side stream / captured step graph, so that a later stream that happens to reuse the handle value cannot pick up
    a buffer the caching allocator still associates with the old stream, and nothing accumulates per stream for the process lifetime."""
    if stream is None:
        _CFG_DECISIONS.clear()
        _ws.clear()
        _splitk_ws.clear()
        _splitk_cnt.clear()
        _proj_cnt.clear()
        for fn in _clear_hooks:
            fn()
        return
    for table in (_ws, _splitk_ws, _splitk_cnt, _proj_cnt):
        for key in [k for k in table if k[-1] == stream]:
            del table[key]


_clear_hooks = []          # modules holding device-side caches of their own register a clearer here (adapter/attention_processor.py)

# ---------------------------------------------------------------------------------------------
# algorithmic FLOP accounting (bench.py: `flops_per_step`): when FLOP_COUNTER is a dict the matrix-shaped wrappers add the
# FLOPs their launch is DEFINED to compute (2 M N K per GEMM / conv, 4 N L d per attention key set; padding excluded).
# ---------------------------------------------------------------------------------------------
FLOP_COUNTER: Optional[dict] = None


def _count(kind: str, flops: float):
    c = FLOP_COUNTER
    if c is not None:
        c[kind] = c.get(kind, 0.0) + float(flops)


def attn_padded_dims(D: int) -> Tuple[int, int]:
    a, b = C.c_int(), C.c_int()
    L.check(L.load().imd_attn_padded_dims(D, C.byref(a), C.byref(b)))
    return a.value, b.value


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------
# Per-shape tile / split-K choices measured on MI355X by tools/gemm_tune.py (like a BLAS tuning file); shapes that
# are not listed fall back to the library heuristic.  Key: "M,N,K,taps,stride,ups".
PATCH_CONV = True          # untabulated 3x3 stride-1 convs on maps >= PATCH_MIN_W wide use the halo-patch kernel (cfg 5)
PATCH_MIN_W = 32
SPLITK_IN_KERNEL = False   # opt-in: K slices summed by each tile's last-arriving workgroup instead of by the finish launch (bit-identical;
                           # measured SLOWER end to end, 660.5 -> 687.5 ms: the slab traffic must bypass the per-XCD L2s)
FUSED_FF = True            # engines run norm3 -> GEGLU feed-forward -> + residual of the 320-channel blocks as one launch (ff_fused.hip)
FUSED_FF_MIN_ROWS = 24576  # below this the 128-row workgroups cannot fill the chip (one per CU at 32768 rows) and the tiled kernels win
import os as _os
FUSED_GN_STATS = _os.environ.get("IMD_FUSED_GN_STATS", "1") != "0"   # 3x3 convs on the halo-patch kernel emit the GroupNorm statistics of their output from the epilogue (A/B switch)
CFG_PAIR_DEDUP = _os.environ.get("IMD_CFG_PAIR_DEDUP", "1") != "0"   # sampling loop: conv_in + first resnet once for the two identical CFG halves (A/B switch)
# A/B only (round 6, measured slower -- DESIGN section 6): GroupNorm + SiLU of a ResNet's 3x3 convolutions applied inside the halo-patch kernel while
# its patch is staged (register-staged form, coefficients from group_norm_coeffs) instead of by a gn_apply launch in front of the LDS-DMA form
FUSED_GN_CONV = _os.environ.get("IMD_FUSED_GN_CONV", "0") == "1"
# (round 6) ResnetBlock2D.norm2 + SiLU inside the finish launch of a K-sliced conv1 (the 16x16 / 8x8 levels): one launch and one HBM round trip less per block.
# OPT-IN: correct and tested, measured neutral at the bench batch (592.0 vs 592.6 ms) and 1.1 % SLOWER at batch 1 (350.8 -> 354.9 ms), same box,
# interleaved twice (profiles/r6h_*): a workgroup per (image, group) reads 160-byte column strips of the fp32 slabs where the plain finish reads whole rows
FUSED_GN_FINISH = _os.environ.get("IMD_FUSED_GN_FINISH", "0") == "1"
# (round 6) Transformer2DModel.norm inside proj_in's row-resident launch (gn_in_*): the normalised tensor never exists in memory (A/B switch)
FUSED_GN_PROJ = _os.environ.get("IMD_FUSED_GN_PROJ", "1") != "0"
# (round 6) the skip concatenation of an up block also writes the GroupNorm statistics of its output: norm1 of the resnet behind it skips its statistics launch (A/B switch)
FUSED_CONCAT_STATS = _os.environ.get("IMD_FUSED_CONCAT_STATS", "1") != "0"
# (round 6) a residual that repeats over the batch (the two halves of a CFG batch) is read in place by the K = 320 row-resident projection instead of being repeated first (A/B switch)
PERIODIC_RES = _os.environ.get("IMD_PERIODIC_RES", "1") != "0"
# (round 6) GroupNorm statistics from the epilogue of the register-staged tile kernel (conv_in, the 64x64-level downsampler, proj_out of the 8x8 level: three
# statistics launches per forward).  OPT-IN: correct and tested, but measured neutral at batch 4 (twelve interleaved pairs: 563.95 vs 563.92 ms) and 0.36 % SLOWER at
# batch 1 (six pairs: 342.7 vs 344.0 ms) -- the reduction at the end of the tile kernel sits on the critical path of launches that do not fill the chip
# (profiles/r6ah_*)
GENERIC_GN_STATS = _os.environ.get("IMD_GENERIC_GN_STATS", "0") == "1"
# (round 6) the pipelines compute the time embeddings of a whole schedule in one pass before the loop (unet._Encoder.precompute_time_embeddings) (A/B switch)
TEMB_TABLE = _os.environ.get("IMD_TEMB_TABLE", "1") != "0"
# ... on which row-resident kernels (A/B): the prologue costs 6-8 us per launch in the running loop (profiles/r6final_kernel_trace_summary.md) -- less than the 10.3 us
# gn_apply launch it replaces at the 64x64 level (tile config 12), about what the 5.4 / 4.3 us launches of the 32x32 / 16x16 levels (13 / 14) cost WITH their launch
# boundary: all levels vs the 64x64 level only measured 593.0 vs 593.0 ms over four pairs (profiles/r6n_*) -> all levels (fewer launches, fewer bytes)
FUSED_GN_PROJ_CFGS = tuple(int(c) for c in _os.environ.get("IMD_FUSED_GN_PROJ_CFGS", "12,13,14").split(",") if c)
CFG_PAIR_ATTN = _os.environ.get("IMD_CFG_PAIR_ATTN", "1") != "0"     # ... and the first hybrid block up to its self-attention phase (unet.Transformer2D.call_pair_half; A/B switch)
FUSED_LN = True            # engines hand `LayerNorm -> attn2.to_q` on 320 channels to the row-resident kernel as ONE launch (A/B switch)
GEMM_TRACE = None          # tools/gemm_tune.py and tests/test_dispatch_sweep_gpu.py set this to a list to record the problems (shape + epilogue) a forward pass launches
GEMM_EVENT_HOOK = None     # tools/insitu_conv.py sets this to a dict: every conv_gemm launch is bracketed by HIP events, keyed by (shape key, cfg, split)
_GEMM_TABLE = None
_CFG_DECISIONS: Dict[Tuple, Tuple[int, int]] = {}      # conv_gemm: problem description -> (tile config, K slices), see there

# ---- per-call tuning (include/imagdressing_hip.h: IMD_TUNING_PER_CALL) ----------------------------------------------------------------
# imd_set_tuning() is process-wide.  Inside ``with tuning_scope(...)`` every params block built by this module carries the scope's choice in
# its `flags` field instead, so two pipelines of one process can run different settings (PipelineBase.set_tuning) and nothing global changes.
TUNING_PER_CALL = 0x5A000000   # 8-bit tag in bits 24..31 (ABI v9): anything else non-zero there is refused by the library
ATTN_VARIANT_MAX = 13      # head-dim-40 variants a product build accepts (14..54 exist in -DIMD_ABLATIONS builds only)


import contextvars

# None | dict(attn_variant=int|None, attn_xcd=bool|None, gemm_flags=int|None).  A ContextVar, not a module global: two pipelines driven from
# two threads (each on its own stream) keep their own scopes -- one thread's __exit__ cannot restore over the other's active scope.
_TUNING = contextvars.ContextVar("imd_tuning_scope", default=None)


class tuning_scope:
    """``with ops.tuning_scope(attn_variant=12, gemm_flags=3): ...`` -- head-dim-40 attention variant (knob 0), XCD-aware attention work
    order (knob 1) and bits 0..4 of the GEMM tuning flags (knob 2) for the launches issued inside, per call.  Scopes nest; None = inherit.
    The scope belongs to the calling thread / context.  It reaches ``ops.conv_gemm`` and ``ops.attention`` only: the fp8 attention, the
    row-resident projections (``row_linear`` / ``row_qkv``) and the fused feed-forward have no per-call choice and ignore it."""

    def __init__(self, attn_variant=None, attn_xcd=None, gemm_flags=None):
        self.new = dict(attn_variant=attn_variant, attn_xcd=attn_xcd, gemm_flags=gemm_flags)

    def __enter__(self):
        merged = dict(_TUNING.get() or {})
        merged.update({k: v for k, v in self.new.items() if v is not None})
        self.token = _TUNING.set(merged if any(v is not None for v in merged.values()) else None)
        return self

    def __exit__(self, *exc):
        _TUNING.reset(self.token)
        return False


def _gemm_call_flags() -> int:
    t = _TUNING.get()
    if t is None or t.get("gemm_flags") is None:
        return 0
    return TUNING_PER_CALL | (int(t["gemm_flags"]) & 31)


def _attn_call_flags() -> int:
    t = _TUNING.get()
    if t is None or (t.get("attn_variant") is None and t.get("attn_xcd") is None):
        return 0
    v = int(t.get("attn_variant") or 0)
    if not 0 <= v <= ATTN_VARIANT_MAX:
        raise L.ImdError(f"tuning_scope: attention variant {v} out of range 0..{ATTN_VARIANT_MAX} (imd_set_tuning(0, .) of the product build)")
    if t.get("attn_xcd") is None:           # inherit the process-wide order
        xcd = bool(L.load().imd_get_tuning(1))
    else:
        xcd = bool(t["attn_xcd"])
    return TUNING_PER_CALL | v | (0 if xcd else 256)


def _gemm_table() -> dict:
    global _GEMM_TABLE
    if _GEMM_TABLE is None:
        import json
        import os
        path = os.environ.get("IMD_GEMM_TUNING") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tuning.json")      # (override: A/B of two tables)
        try:
            with open(path) as f:
                _GEMM_TABLE = json.load(f).get("shapes", {})
        except FileNotFoundError:
            _GEMM_TABLE = {}
    return _GEMM_TABLE


# ---- tile configs on the dispatcher's side (what a config number IS -- tile, launcher, K-slice finish, statistics epilogue -- is the library's table,
# csrc/conv_gemm.hip::TILE_CONFIGS): how a tabulated entry is re-validated, and which configs the fusions below may use -------------------------------
def _conv_dma_ok(bk: int):      # Python copy of gemm_dma.hip::imd_conv_dma_supported (not exported): 3x3 convs gathered per tile, ``bk`` channels at a time
    return lambda p: p.taps == 9 and p.Cin % bk == 0 and p.stride in (1, 2) and not p.gn_a


ROW_RESIDENT_CFGS = (12, 13, 14)            # the row-resident projections (K = 320 / 640 / 1280): the ones with a gn_in prologue
# tile config -> the library query (or predicate over the parameter block) a tabulated entry must pass: the table is keyed by (M, N, K, taps, stride, ups)
# only, and another geometry with the same key (W % 16 != 0, pad_br_only, strided pixels ...) may not qualify; the register-staged tiles take anything
TILE_SUPPORT = {5: "imd_conv_patch_supported", 21: "imd_conv_patch2_supported", 22: "imd_conv_patch3_supported", 23: "imd_conv_patch4_supported",
                24: "imd_conv_img_supported", **{c: "imd_row_linear_supported" for c in ROW_RESIDENT_CFGS + (15,)},
                **{c: "imd_gemm_dma_supported" for c in (16, 17, 19, 25, 27, 30, 31, 32)},
                18: _conv_dma_ok(32), 20: _conv_dma_ok(32), 26: _conv_dma_ok(64), 28: _conv_dma_ok(64)}
SLICES_ONLY_CFGS = frozenset({24})          # whole-map kernel of the 8-wide levels: K-sliced only, so its query is asked with the tabulated K slices in the block
PATCH_CFG = 5                               # the halo-patch kernel: the road of untabulated 3x3 stride-1 convs on wide maps, and the one with the ``gn`` prologue
PERIODIC_RES_CFGS = frozenset({12})         # read a periodic residual in place (res_rows)
STATS_EPILOGUE_CFGS = frozenset({5, 22, 23, 29})            # halo-patch kernels: un-split epilogues that write the GroupNorm statistics of their output
TILE_STATS_CFGS = frozenset({-1, 0, 1, 2, 3, 4, 7})         # register-staged tiles that do (GENERIC_GN_STATS); -1: the library heuristic picks among them


def _marshal(x, w, M, N, K, Cin, taps, Hin, Win, Hout, Wout, stride, ups, x_pix_stride, out, out_ld, bias, rowvec, rowvec_stride, rowvec_off, res, res_ld,
             out_scale, act, out_f32, heads, pad_br_only):
    """-> (the parameter block of the problem, tile choice and fusions still open; the output tensor; rows of a periodic residual or 0)."""
    p = L.ConvGemmParams()
    p.flags = _gemm_call_flags()
    dt = x.dtype
    p.dtype, p.x, p.w = _code(x, "x"), _dev(x, dt, "x"), _dev(w, dt, "w")
    if w.numel() != N * K:
        raise L.ImdError(f"conv_gemm: weight has {w.numel()} elements, expected N*K = {N}*{K}")
    p.M, p.N, p.K = M, N, K
    p.Cin, p.taps, p.Hin, p.Win, p.Hout, p.Wout, p.stride, p.ups = Cin, taps, Hin, Win, Hout, Wout, stride, int(ups)
    p.x_pix_stride = Cin if x_pix_stride is None else x_pix_stride
    p.bias = None if bias is None else _dev(bias, torch.float32, "bias")
    p.rowvec = None if rowvec is None else _dev(rowvec, torch.float32, "rowvec")
    if rowvec is not None and rowvec_off:
        if rowvec_off % 4:
            raise L.ImdError("conv_gemm: rowvec_off must be a multiple of 4")
        p.rowvec = p.rowvec + 4 * rowvec_off
    p.rowvec_stride, p.res, p.res_ld = rowvec_stride, None if res is None else _dev(res, dt, "res"), N if res_ld is None else res_ld
    # a residual with FEWER rows than the output is periodic (row m adds res[m % rows]): one copy of a tensor that is the same for both halves of a
    # CFG batch.  The K = 320 row-resident projection reads it in place (res_rows); everywhere else it is repeated into a full-size tensor first.
    res_rows = 0
    if res is not None and res_ld is None and res.numel() != M * N:
        res_rows = res.numel() // N
        if res_rows <= 0 or res_rows * N != res.numel() or M % res_rows:
            raise L.ImdError(f"conv_gemm: the residual has {res.numel()} elements: neither M x N = {M} x {N} nor a whole divisor of it")
    p.out_scale, p.pad_br_only, p.act, p.out_f32 = out_scale, int(pad_br_only), act, int(out_f32)
    if heads is not None:
        p.mode = 1
        p.hC, p.hH, p.hD = heads["C"], heads["H"], heads["D"]
        for i, (t, kind, DP, Ltok, scale) in enumerate(heads["dests"]):
            p.hd[i].ptr = None if t is None else _dev(t, dt, f"heads[{i}]")
            p.hd[i].kind, p.hd[i].DP, p.hd[i].L, p.hd[i].scale = kind, DP, Ltok, scale
        p.out, p.out_ld = None, 0
    else:
        p.mode = 0
        n_out = N // 2 if act == ACT_GEGLU else N
        if out is None:
            out = torch.empty((M, n_out), dtype=torch.float32 if out_f32 else dt, device=x.device)
        p.out = _dev(out, torch.float32 if out_f32 else dt, "out")
        p.out_ld = n_out if out_ld is None else out_ld
    return p, out, res_rows


def _choose_tile(p, lib, cfg: int, split_k: int, splittable: bool) -> Tuple[int, int]:
    """(tile config, K slices) where the caller left them open (-1 / 0): the tuning table, re-validated through TILE_SUPPORT, else the halo-patch kernel or
    the library heuristic (-1); the library's K-slice count.  Reads the parameter block and the table only, no tensors: conv_gemm remembers the answer."""
    if cfg == -1 and split_k == 0:
        # 3x3 convs are keyed WITH their output map as well: the same (M, N, K) occurs for different maps (2 images of 20x16 and 8 of 10x8 are both 640 rows)
        key = f"{p.M},{p.N},{p.K},{p.taps},{p.stride},{p.ups}"
        ent = (_gemm_table().get(f"{key}|{p.Hout}x{p.Wout}") if p.taps == 9 else None) or _gemm_table().get(key)
        if ent is not None:
            cfg, split_k = (ent["cfg"], ent["split"]) if splittable else (ent["cfg_nosplit"], 1)
            ok = TILE_SUPPORT.get(cfg)
            if cfg in SLICES_ONLY_CFGS:
                p.split_k = split_k
            if ok is not None and not (getattr(lib, ok)(C.byref(p)) if isinstance(ok, str) else ok(p)):
                cfg, split_k = -1, 0        # back to the library heuristic
    # off the measured table 3x3 stride-1 convs on wide maps go to the halo-patch kernel (always ahead of the gather kernel there: profiles/r1k_patch_conv_ab.jsonl)
    if PATCH_CONV and cfg == -1 and p.taps == 9 and p.stride == 1 and p.Wout >= PATCH_MIN_W and p.N >= 64 and lib.imd_conv_patch_supported(C.byref(p)):
        cfg = PATCH_CFG
    if split_k == 0:        # auto: K slices only where the tile grid cannot fill the chip
        split_k = 1 if not splittable else lib.imd_conv_gemm_auto_split(p.M, p.N, p.K, cfg)
    return cfg, split_k


def _periodic_residual(p, res, res_rows: int, in_place: bool):       # -> the residual the launch reads (the caller keeps it alive)
    if in_place and res_rows % 128 == 0 and PERIODIC_RES:
        p.res_rows = res_rows
        return res
    res = repeat_batch(res.reshape(res_rows, p.N), p.M // res_rows)
    p.res = _dev(res, res.dtype, "res")
    return res


def _fuse_gn_in(p, lib, x, gn_in, cfg: int, M: int, HW: int):
    """``gn_in`` = (gamma, beta, eps, silu, groups), Transformer2DModel.norm -> proj_in: where the layer runs on a row-resident projection kernel and ``x`` carries
    its producer's statistics (``_imd_gn_stats``) the normalisation happens inside that launch (``imd_conv_gemm_params.gn_in_*``: bit-identical, no normalised
    tensor in memory); everywhere else :func:`group_norm` runs first.  -> the normalised tensor ``p.x`` then points to (the caller keeps it alive), or None."""
    gamma, beta, eps, silu, groups = gn_in
    st = getattr(x, "_imd_gn_stats", None)
    if FUSED_GN_PROJ and cfg in FUSED_GN_PROJ_CFGS and st is not None and st[2] == groups and FUSED_GN_STATS and st[0].shape[0] * HW == M:
        p.gn_in_partial, p.gn_in_nparts, p.gn_in_groups = st[0].data_ptr(), st[1], int(groups)
        p.gn_in_gamma, p.gn_in_beta = _dev(gamma, torch.float32, "gn_in gamma"), _dev(beta, torch.float32, "gn_in beta")
        p.gn_in_eps, p.gn_in_silu = float(eps), int(bool(silu))
        if lib.imd_row_linear_gn_in_supported(C.byref(p), cfg):
            return None
        p.gn_in_partial, p.gn_in_nparts, p.gn_in_groups = None, 0, 0
    xv = x.view(M // HW, HW, p.Cin)
    if st is not None:
        xv._imd_gn_stats = st
    xn = group_norm(xv, gamma, beta, groups=groups, eps=eps, silu=silu)
    p.x = _dev(xn, x.dtype, "x")
    return xn


def _fuse_gn_out(p, lib, gn_out, out_scale: float) -> bool:
    """``gn_out`` = (gamma, beta, eps, silu, groups), ResnetBlock2D: conv1 -> norm2 -> SiLU: where the problem is K-sliced with a separate finish launch that can own whole
    (image, group) slabs (``imd_conv_gemm_gn_out_supported``: the 16x16 / 8x8 levels) it normalises its output itself: gn_out_* filled in and True.  Else the block as it was, False."""
    gamma, beta, eps, silu, groups = gn_out
    if not (p.split_k > 1 and p.mode == 0 and not p.out_f32 and p.act == ACT_NONE and not p.res and out_scale == 1.0):
        return False
    p.gn_out_gamma, p.gn_out_beta = _dev(gamma, torch.float32, "gn_out gamma"), _dev(beta, torch.float32, "gn_out beta")
    p.gn_out_eps, p.gn_out_silu, p.gn_out_groups = float(eps), int(bool(silu)), int(groups)
    if lib.imd_conv_gemm_gn_out_supported(C.byref(p)):
        p.splitk_counters = None
        return True
    p.gn_out_gamma, p.gn_out_beta, p.gn_out_groups = None, None, 0
    return False


def _attach_stats(p, lib, cfg: int, split_k: int, groups: int, images: int, device):
    """GroupNorm(``groups``) statistics of the OUTPUT as per-tile / per-pixel-part fp32 partials: from the epilogue (halo-patch kernels un-split; with
    GENERIC_GN_STATS the register-staged tiles -- conv_in, the stride-2 downsampler of the 64x64 level -- wherever a tile's rows lie in one image) or from
    the finish launch of the K slices (row-major 16-bit outputs).  gn_stats_* filled in -> (partials [images, nparts, groups, 2], nparts, groups), or None where this launch cannot."""
    if not (cfg in STATS_EPILOGUE_CFGS or split_k > 1 or (GENERIC_GN_STATS and cfg in TILE_STATS_CFGS)):
        return None
    p.gn_stats_groups = groups
    nparts = lib.imd_conv_gemm_stats_parts(C.byref(p), cfg)
    if nparts <= 0:
        p.gn_stats_groups = 0
        return None
    part = torch.empty((images, nparts, groups, 2), dtype=torch.float32, device=device)
    p.gn_stats_out = part.data_ptr()
    return part, nparts, groups


def conv_gemm(
    x: torch.Tensor, w: torch.Tensor, *, M: int, N: int, Cin: int, taps: int = 1,
    Hin: int = 1, Win: int = 1, Hout: int = 1, Wout: int = 1, stride: int = 1, ups: bool = False,
    x_pix_stride: Optional[int] = None, out: Optional[torch.Tensor] = None, out_ld: Optional[int] = None,
    bias: Optional[torch.Tensor] = None, rowvec: Optional[torch.Tensor] = None, rowvec_stride: int = 0,
    rowvec_off: int = 0, res: Optional[torch.Tensor] = None, res_ld: Optional[int] = None, out_scale: float = 1.0,
    act: int = ACT_NONE, out_f32: bool = False, heads: Optional[dict] = None, cfg: int = -1, split_k: int = 0,
    gn: Optional[tuple] = None, pad_br_only: bool = False, ln_eps: Optional[float] = None, gn_stats_groups: int = 0,
    gn_out: Optional[tuple] = None, gn_in: Optional[tuple] = None,
) -> Optional[torch.Tensor]:
    """out[M, N] = epilogue(A(M, K) @ w[N, K]^T); see include/imagdressing_hip.h::imd_conv_gemm.

    ``heads`` = dict(C=, H=, D=, dests=[(tensor|None, kind, DP, L, scale), ...]) selects the head-split epilogue (no ``out``).  Returns the output tensor (allocated when ``out`` is None).
    ``gn`` = (coef_a [B, Cin] fp32, coef_b [B, Cin] fp32, silu) from :func:`group_norm_coeffs` fuses GroupNorm(+SiLU) of the input into the 3x3 halo-patch kernel (tile config 5).
    ``ln_eps``: LayerNorm WITHOUT affine over the K channels of every row of ``x`` is applied on the fly (row-resident kernel, K = 320 and N <= 320 only; fold gamma / beta into ``w`` / ``bias`` with :func:`fold_layernorm_affine`).
    ``gn_in``: GroupNorm (+ SiLU) of the INPUT ``x`` [B, HW, K] of a plain linear layer, inside the launch where it can be (:func:`_fuse_gn_in`).
    ``gn_out``: GroupNorm (+ SiLU) of the OUTPUT inside the finish launch of the K slices where that exists (:func:`_fuse_gn_out`); the returned tensor then
    carries ``_imd_gn_applied = True`` and holds the NORMALISED values.  Ignored (raw output) everywhere else.
    ``gn_stats_groups`` = G: where the launch can (:func:`_attach_stats`) it also writes the GroupNorm(G) statistics of the OUTPUT; they ride on the returned tensor
    (``_imd_gn_stats``) and the next :func:`group_norm` of that tensor skips its statistics pass.  Silently not produced on every other path (FUSED_GN_STATS = False: never).
    """
    ensure_device(x.device)
    K = taps * Cin
    p, out, res_rows = _marshal(x, w, M, N, K, Cin, taps, Hin, Win, Hout, Wout, stride, ups, x_pix_stride, out, out_ld, bias, rowvec, rowvec_stride, rowvec_off,
                                res, res_ld, out_scale, act, out_f32, heads, pad_br_only)
    _count("gemm_conv", 2.0 * M * N * K)
    lib = L.load()
    if gn is not None:
        p.gn_a, p.gn_b, p.gn_silu = _dev(gn[0], torch.float32, "gn_a"), _dev(gn[1], torch.float32, "gn_b"), int(gn[2])
        if cfg == -1:
            cfg = PATCH_CFG
    if ln_eps is not None:
        if res_rows:
            res = _periodic_residual(p, res, res_rows, K == 320)
        p.split_k = 1
        L.check(lib.imd_row_linear(C.byref(p), 1, float(ln_eps), _stream()))
        return out
    splittable = heads is None and act != ACT_GEGLU
    if GEMM_TRACE is not None:
        GEMM_TRACE.append(dict(M=M, N=N, K=K, Cin=Cin, taps=taps, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=stride, ups=int(ups), splittable=splittable, dtype=str(x.dtype),
                               # the epilogue, so that a traced problem can be replayed standalone (tests/test_dispatch_sweep_gpu.py)
                               bias=bias is not None, rowvec=rowvec is not None, rowvec_stride=rowvec_stride, res=res is not None, res_rows=res_rows, act=act, out_f32=bool(out_f32),
                               heads=None if heads is None else dict(C=heads["C"], H=heads["H"], D=heads["D"],
                                                                     dests=[(t is not None, kind, DP, Ltok, scale) for t, kind, DP, Ltok, scale in heads["dests"]]),
                               gn_stats_groups=gn_stats_groups, x_pix_stride=p.x_pix_stride, out_scale=out_scale, pad_br_only=bool(pad_br_only),
                               out_ld=p.out_ld, res_ld=p.res_ld, gn=gn is not None, gn_in=gn_in is not None, gn_out=gn_out is not None))
    # (round 6) the (tile config, K slices) decision of a call site is a pure function of the problem description: remembered per description, so
    # that a repeated layer pays neither the table key formatting nor the library's *_supported queries again (~5 of the ~75 us a processor call
    # costs on the host at the small levels).  Dropped with the tuning table (IMD_GEMM_TUNING / _GEMM_TABLE reset) and by clear_workspaces().
    dkey = hit = None
    if cfg == -1 and split_k == 0 and GEMM_TRACE is None:
        hk = None if heads is None else (heads["C"], heads["H"], heads["D"], tuple((t is None, kind, DP, Ltok) for t, kind, DP, Ltok, _ in heads["dests"]))
        dkey = (M, N, K, Cin, taps, stride, int(ups), Hin, Win, Hout, Wout, p.x_pix_stride, p.res_ld, p.out_ld, act, int(out_f32), int(pad_br_only), p.dtype,
                rowvec is None, res is None, bias is None, hk, PATCH_CONV, id(_GEMM_TABLE))
        hit = _CFG_DECISIONS.get(dkey)
    cfg, split_k = hit or _choose_tile(p, lib, cfg, split_k, splittable)
    if hit is None and dkey is not None and len(_CFG_DECISIONS) < 4096:
        _CFG_DECISIONS[dkey] = (cfg, split_k)
    if res_rows:
        res = _periodic_residual(p, res, res_rows, cfg in PERIODIC_RES_CFGS)
    p.split_k = split_k
    xn = None if gn_in is None else _fuse_gn_in(p, lib, x, gn_in, cfg, M, Hout * Wout)      # noqa: F841  (kept alive until the launch is issued)
    if split_k > 1:
        p.splitk_ws = splitk_workspace(split_k * M * N, x.device).data_ptr()
        if SPLITK_IN_KERNEL:
            p.splitk_counters = splitk_counters(x.device).data_ptr()
    if gn_out is not None and FUSED_GN_FINISH and _fuse_gn_out(p, lib, gn_out, out_scale):
        L.check(lib.imd_conv_gemm(C.byref(p), cfg, _stream()))
        out._imd_gn_applied = True          # the caller skips its own group_norm
        return out
    stats = None
    if gn_stats_groups and FUSED_GN_STATS and heads is None and not out_f32 and act != ACT_GEGLU:
        stats = _attach_stats(p, lib, cfg, split_k, gn_stats_groups, M // (Hout * Wout), x.device)
    if GEMM_EVENT_HOOK is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.imd_conv_gemm(C.byref(p), cfg, _stream()))
        e1.record()
        GEMM_EVENT_HOOK.setdefault((f"{M},{N},{K},{taps},{stride},{int(ups)}|{Hout}x{Wout}", cfg, split_k), []).append((e0, e1))
    else:
        L.check(lib.imd_conv_gemm(C.byref(p), cfg, _stream()))
    if stats is not None:
        out._imd_gn_stats = stats
    return out


_splitk_ws: Dict[Tuple, torch.Tensor] = {}
_splitk_cnt: Dict[Tuple, torch.Tensor] = {}


def splitk_counters(device) -> torch.Tensor:
    """Zeroed per-tile arrival counters of the in-kernel split-K reduction (include/imagdressing_hip.h::splitk_counters); every
    launch leaves them zero, launches are stream-ordered, so one array per device serves all of them."""
    key = (str(device), _stream())
    t = _splitk_cnt.get(key)
    if t is None:
        t = torch.zeros(16384, dtype=torch.int32, device=device)
        _splitk_cnt[key] = t
    return t


def splitk_workspace(nfloats: int, device) -> torch.Tensor:
    """Grow-only fp32 scratch for split-K partial tiles (stream-ordered reuse: one per device AND stream)."""
    key = (str(device), _stream())
    t = _splitk_ws.get(key)
    if t is None or t.numel() < nfloats:
        t = torch.empty(max(nfloats, 1 << 22), dtype=torch.float32, device=device)
        _splitk_ws[key] = t
    return t


def linear(x2d: torch.Tensor, w: torch.Tensor, bias=None, *, res=None, act=ACT_NONE, out_f32=False, out=None,
           out_ld=None, res_ld=None, cfg=-1, split_k=0, ln_eps=None) -> torch.Tensor:
    M, K = x2d.shape
    N = w.shape[0]
    return conv_gemm(x2d, w, M=M, N=N, Cin=K, bias=bias, res=res, act=act, out_f32=out_f32, out=out,
                     out_ld=out_ld, res_ld=res_ld, cfg=cfg, split_k=split_k, ln_eps=ln_eps)


def fold_layernorm_affine(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """(W', b') with  LN_affine(x) @ W^T + b == LN_plain(x) @ W'^T + b':  W' = W diag(gamma) (rounded once to the weight dtype),
    b' = b + W beta (fp32).  Host-side, once per layer (``ln_eps`` of :func:`conv_gemm`)."""
    wf = w.float()
    w2 = (wf * gamma.float()[None, :]).to(w.dtype).contiguous()
    b2 = wf @ beta.float()
    if bias is not None:
        b2 = b2 + bias.float()
    return w2, b2.contiguous()


def pack_ff_fused(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, gamma: Optional[torch.Tensor] = None,
                  beta: Optional[torch.Tensor] = None, dtype=None):
    """Operands of :func:`ff_geglu_fused` from the diffusers-layout FeedForward parameters: ``w1`` [2*inner, C] / ``b1`` =
    ff.net.0.proj (rows [0, inner) = value, [inner, 2*inner) = gate: ``hidden, gate = proj(x).chunk(2, -1)``), ``w2`` [C, inner] /
    ``b2`` = ff.net.2; ``gamma`` / ``beta`` = norm3, folded into w1 / b1 (the kernel normalises without affine).  Layout: see
    include/imagdressing_hip.h::imd_ff_params.  Host-side, once per layer."""
    dtype = dtype or w1.dtype
    inner, C = w2.shape[1], w2.shape[0]
    w1f, b1f = w1.float(), b1.float()
    if gamma is not None:
        b1f = b1f + w1f @ beta.float()
        w1f = w1f * gamma.float()[None, :]
    dev = w1.device
    i = torch.arange(32, device=dev)
    jj = (i & 7) + 8 * (i >> 4)                                  # inner channel of packed row i inside its 16-block
    gate = ((i >> 3) & 1).bool()
    blk = torch.arange(inner // 16, device=dev)
    src = 16 * blk[:, None] + jj[None, :] + torch.where(gate, inner, 0)[None, :]          # [blocks, 32] rows of w1
    w1p = w1f[src.reshape(-1)].to(dtype).contiguous()            # [blocks * 32, C]
    b1p = b1f[src.reshape(-1)].contiguous()
    ks = torch.arange(16, device=dev)
    jk = torch.where(ks < 4, ks, torch.where(ks < 8, ks + 4, torch.where(ks < 12, ks - 4, ks)))     # slot -> inner channel in the 16-group
    cols = (16 * torch.arange(inner // 16, device=dev)[:, None] + jk[None, :]).reshape(inner // 32, 32)     # [chunks, 32]
    w2p = w2.float()[:, cols].permute(1, 0, 2).to(dtype).contiguous()                     # [chunks, C, 32]
    return dict(w1=w1p, b1=b1p, w2=w2p, b2=b2.float().contiguous(), ln=gamma is not None, C=C, inner=inner)


def ff_geglu_fused(x2d: torch.Tensor, packed: dict, ln_eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x + b2 + W2 geglu(W1 LN(x) + b1) in one launch (include/imagdressing_hip.h::imd_ff_geglu; C = 320, inner = 1280)."""
    ensure_device(x2d.device)
    M, C_ = x2d.shape
    dt = x2d.dtype
    if out is None:
        out = torch.empty((M, C_), dtype=dt, device=x2d.device)
    p = L.FfParams()
    p.x, p.w1, p.b1 = _dev(x2d, dt, "x"), _dev(packed["w1"], dt, "w1"), _dev(packed["b1"], torch.float32, "b1")
    p.w2, p.b2, p.out = _dev(packed["w2"], dt, "w2"), _dev(packed["b2"], torch.float32, "b2"), _dev(out, dt, "out")
    p.M, p.C, p.inner, p.x_ld, p.out_ld = M, packed["C"], packed["inner"], x2d.stride(0), out.stride(0)
    p.ln, p.ln_eps, p.dtype = int(packed["ln"]), float(ln_eps), _code(x2d, "x")
    _count("gemm_conv", 2.0 * M * packed["C"] * 2 * packed["inner"] + 2.0 * M * packed["inner"] * packed["C"])
    L.check(L.load().imd_ff_geglu(C.byref(p), _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Text cross-attention of a 320-channel block as one launch (csrc/row_xattn.hip; include/imagdressing_hip.h::imd_xattn_params):
# norm2 -> attn2.to_q -> softmax(q Kt^T) Vt over <= 96 text keys -> attn2.to_out[0] + bias + residual.  A/B switch, default on.
# ---------------------------------------------------------------------------------------------------------------------
FUSED_XATTN = _os.environ.get("IMD_FUSED_XATTN", "1") != "0"
XATTN_C, XATTN_HEADS, XATTN_D, XATTN_DP, XATTN_LMAX = 320, 8, 40, 48, 96
XATTN_CHUNK = 64 * 320                 # elements of one LDS ring slot (40960 bytes)
XATTN_VROW = 104                       # elements of a V^T image row: 96 key columns + one 16-byte piece of padding
XATTN_HEAD = XATTN_LMAX * XATTN_DP + XATTN_DP * XATTN_VROW       # 9600 elements: K image, then V^T image
XATTN_PAD_KEY = -30000.0               # K column 40 of a pad key (exact in fp16): exp2(score - max) is 0 in fp32
_XATTN_W: Dict[Tuple, tuple] = {}
_XATTN_KV: Dict[int, tuple] = {}
_clear_hooks.append(_XATTN_W.clear)
_clear_hooks.append(_XATTN_KV.clear)


def xattn_q_rows(device=None):
    """(source row of W_q' [384], valid [384]) of the packed to_q rows: packed row 64 c + r belongs to wave half r // 32, whose row
    R = 32 c + r % 32 is dim R % 48 of head 4 (r // 32) + R // 48 (dims 40..47: zero rows)."""
    i = torch.arange(6 * 64, device=device)
    r = i % 64
    R = 32 * (i // 64) + r % 32
    head, dim = 4 * (r // 32) + R // 48, R % 48
    return head * XATTN_D + dim.clamp(max=XATTN_D - 1), dim < XATTN_D


def xattn_o_cols(device=None):
    """Source column of W_o [320] at packed input position 16 s + 8 hi + e: channel group 2 s + e // 4 of the list (head h, group j) ->
    5 h + j, dim 8 j + 4 hi + e % 4 -- the order in which a lane's O registers leave the P.V accumulators."""
    k = torch.arange(XATTN_C, device=device)
    s, hi, e = k // 16, (k % 16) // 8, k % 8
    G = 2 * s + e // 4
    return (G // 5) * XATTN_D + 8 * (G % 5) + 4 * hi + e % 4


def xattn_swizzle_rows(w2d: torch.Tensor) -> torch.Tensor:
    """[R, 320] -> the same rows as they sit in an LDS ring slot: the 16-byte piece at position q of chunk row r is source piece
    q ^ ((r >> 1) & 7) (r = row % 64).  An involution."""
    R = w2d.shape[0]
    r = torch.arange(R, device=w2d.device) % 64
    pos = torch.arange(40, device=w2d.device)[None, :] ^ ((r >> 1) & 7)[:, None]
    return w2d.reshape(R, 40, 8).gather(1, pos[:, :, None].expand(R, 40, 8)).reshape(R, XATTN_C).contiguous()


def xattn_key_cols(device=None):
    """Key held by column c of a V^T image: inside every 16-key step the keys sit in the register order of an S^T accumulator
    (0-3, 8-11, 4-7, 12-15), so that packed P registers are the B operand of O^T += V^T P^T."""
    c = torch.arange(XATTN_LMAX, device=device)
    c16 = c % 16
    return (c // 16) * 16 + (c16 & 3) + 8 * ((c16 >> 2) & 1) + 4 * (c16 >> 3)


def xattn_k_pieces(device=None):
    """[96, 6]: source 16-byte piece at position q of K image row r (rows 8..15 mod 16 are stored rotated by three pieces)."""
    r = torch.arange(XATTN_LMAX, device=device)
    return (torch.arange(6, device=device)[None, :] - 3 * ((r >> 3) & 1)[:, None]) % 6


def _pack_text_xattn(wq, bq, wo, bo):
    dev, dt = wq.device, wq.dtype
    src, valid = xattn_q_rows(dev)
    wq_p = torch.where(valid[:, None], wq[src], torch.zeros((), dtype=dt, device=dev))
    bq_p = torch.where(valid, bq.float()[src], torch.zeros((), dtype=torch.float32, device=dev)).contiguous()
    wo_p = wo[:, xattn_o_cols(dev)]
    w = torch.cat([xattn_swizzle_rows(wq_p), xattn_swizzle_rows(wo_p)], 0).contiguous()
    bo_p = torch.zeros(XATTN_C, dtype=torch.float32, device=dev) if bo is None else bo.float().contiguous()
    return dict(w=w, bq=bq_p, bo=bo_p)


def pack_text_xattn(wq: torch.Tensor, bq: torch.Tensor, wo: torch.Tensor, bo: Optional[torch.Tensor]):
    """Weights of :func:`text_xattn` from ``wq`` [320, 320] / ``bq`` [320] fp32 (LayerNorm affine folded in:
    :func:`fold_layernorm_affine`) and ``wo`` [320, 320] / ``bo`` [320] fp32 | None.  Layout: include/imagdressing_hip.h::imd_xattn_params.
    Host-side, once per layer: cached against the storage and version of the four tensors (which the cache keeps alive)."""
    if tuple(wq.shape) != (XATTN_C, XATTN_C) or tuple(wo.shape) != (XATTN_C, XATTN_C) or wq.dtype != wo.dtype:
        raise L.ImdError(f"pack_text_xattn: expected two [320, 320] matrices of one dtype, got {tuple(wq.shape)} {wq.dtype}, {tuple(wo.shape)} {wo.dtype}")
    srcs = (wq, bq, wo, bo)
    key = tuple(None if t is None else (t.data_ptr(), t._version, t.dtype, str(t.device)) for t in srcs)
    ent = _XATTN_W.get(key)
    if ent is None:
        if len(_XATTN_W) > 64:
            _XATTN_W.clear()
        ent = _XATTN_W[key] = (srcs, _pack_text_xattn(wq, bq, wo, bo))
    return ent[1]


def _pack_text_kv(k, vt, Lk):
    Bt, dev, dt = k.shape[0], k.device, k.dtype
    H, D, DP, LM = XATTN_HEADS, XATTN_D, XATTN_DP, XATTN_LMAX
    kf = torch.zeros(Bt, H, LM, DP, dtype=dt, device=dev)
    kf[:, :, :Lk, :D] = k[:, :, :Lk, :D]
    kf[:, :, Lk:, D] = XATTN_PAD_KEY
    kimg = kf.view(Bt, H, LM, 6, 8).gather(3, xattn_k_pieces(dev)[None, None, :, :, None].expand(Bt, H, LM, 6, 8))
    vf = torch.zeros(Bt, H, DP, LM, dtype=dt, device=dev)
    vf[:, :, :D, :Lk] = vt[:, :, :D, :Lk]
    vf[:, :, D, :] = 1.0
    vimg = torch.zeros(Bt, H, DP, XATTN_VROW, dtype=dt, device=dev)
    vimg[..., :LM] = vf[..., xattn_key_cols(dev)]
    head = torch.cat([kimg.reshape(Bt, H, LM * DP), vimg.reshape(Bt, H, DP * XATTN_VROW)], -1)
    img = torch.zeros(Bt, 4, XATTN_CHUNK, dtype=dt, device=dev)
    img[:, :, :XATTN_HEAD] = head[:, :4]
    img[:, :, XATTN_HEAD:2 * XATTN_HEAD] = head[:, 4:]
    return img


def pack_text_kv(k: torch.Tensor, vt: torch.Tensor, Lk: int) -> torch.Tensor:
    """K / V^T images of :func:`text_xattn` [Bt, 4, 20480] from the projected text keys ``k`` [Bt, 8, Lk, 48] and values
    ``vt`` [Bt, 8, 64, LP] (the operands of :func:`attention`): chunk c = heads c and c + 4 exactly as they sit in an LDS ring slot --
    K [96 keys][48 dims] with column 40 = 0 (key) / XATTN_PAD_KEY (pad key), V^T [48][104] with an all-ones row 40 and the key
    columns in accumulator order.  Step-invariant: built once per projected K (cached against its identity, which the cache keeps
    alive) and dropped by :func:`clear_workspaces`."""
    if k.dim() != 4 or k.shape[1] != XATTN_HEADS or k.shape[3] != XATTN_DP or not (1 <= Lk <= XATTN_LMAX) or k.shape[2] < Lk \
            or vt.shape[:2] != k.shape[:2] or vt.shape[2] < XATTN_D or vt.shape[3] < Lk:
        raise L.ImdError(f"pack_text_kv: expected K [Bt, 8, L, 48] / V^T [Bt, 8, >= 40, >= L] with L <= 96, got {tuple(k.shape)} / {tuple(vt.shape)}, L = {Lk}")
    hit = _XATTN_KV.get(id(k))
    if hit is not None and hit[0] is k and hit[1] is vt and hit[2] == Lk:
        return hit[3]
    if len(_XATTN_KV) > 64:
        _XATTN_KV.clear()
    img = _pack_text_kv(k, vt, Lk)
    _XATTN_KV[id(k)] = (k, vt, Lk, img)
    return img


def text_xattn_supported(C_: int, heads: int, N: int, Lk: int) -> bool:
    return C_ == XATTN_C and heads == XATTN_HEADS and N % 128 == 0 and 1 <= Lk <= XATTN_LMAX


def text_xattn(x: torch.Tensor, packed: dict, kv_img: torch.Tensor, *, Lk: int, kv_bdiv: int = 1, ln_eps: float = 1e-5,
               q_scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x + bo + Wo attention(LN(x) Wq'^T + bq', text K / V) for ``x`` [B, N, 320] in one launch
    (include/imagdressing_hip.h::imd_text_xattn320).  ``packed`` = :func:`pack_text_xattn`, ``kv_img`` = :func:`pack_text_kv` of the
    B / kv_bdiv conditioning rows.  No allocation besides ``out``, no synchronisation."""
    ensure_device(x.device)
    B, N, C_ = x.shape
    dt = x.dtype
    if out is None:
        out = torch.empty((B, N, C_), dtype=dt, device=x.device)
    if kv_img.dim() != 3 or tuple(kv_img.shape[1:]) != (4, XATTN_CHUNK):
        raise L.ImdError(f"text_xattn: kv_img must be [Bt, 4, {XATTN_CHUNK}], got {tuple(kv_img.shape)}")
    p = L.XattnParams()
    p.x, p.w, p.out = _dev(x, dt, "x"), _dev(packed["w"], dt, "w"), _dev(out, dt, "out")
    p.bq, p.bo, p.kv = _dev(packed["bq"], torch.float32, "bq"), _dev(packed["bo"], torch.float32, "bo"), _dev(kv_img, dt, "kv_img")
    p.M, p.C, p.heads, p.L = B * N, C_, XATTN_HEADS, int(Lk)
    p.rows_per_image, p.kv_bdiv, p.text_rows = N, int(kv_bdiv), kv_img.shape[0]
    p.x_ld = p.out_ld = C_
    p.q_scale = float(XATTN_D ** -0.5 * 1.4426950408889634 if q_scale is None else q_scale)
    p.ln_eps, p.dtype = float(ln_eps), _code(x, "x")
    _count("gemm_conv", 2 * 2.0 * B * N * C_ * C_)
    _count("attention", 4.0 * XATTN_HEADS * N * XATTN_D * B * Lk)
    L.check(L.load().imd_text_xattn320(C.byref(p), _stream()))
    return out


def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, bias=None, *, taps=9, stride=1, ups=False, rowvec=None,
                rowvec_stride=0, rowvec_off=0, res=None, out_scale=1.0, act=ACT_NONE, out_f32=False, cfg=-1, split_k=0, gn=None,
                pad_br_only=False, gn_stats_groups=0, gn_out=None, gn_in=None) -> torch.Tensor:
    """x [B, H, W, Cin] bf16 -> [B, Ho, Wo, Cout].  ``pad_br_only``: F.pad(x, (0, 1, 0, 1)) + conv(padding=0) (VAE encoder)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Hl, Wl = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = ((Hl + stride - 1) // stride, (Wl + stride - 1) // stride)
    M = B * Ho * Wo
    out = conv_gemm(x, w, M=M, N=Cout, Cin=Cin, taps=taps, Hin=H, Win=W, Hout=Ho, Wout=Wo, stride=stride, ups=ups,
                    bias=bias, rowvec=rowvec, rowvec_stride=rowvec_stride, rowvec_off=rowvec_off, res=res, out_scale=out_scale, act=act,
                    out_f32=out_f32, cfg=cfg, split_k=split_k, gn=gn, pad_br_only=pad_br_only, gn_stats_groups=gn_stats_groups, gn_out=gn_out, gn_in=gn_in)
    r = out.view(B, Ho, Wo, -1)
    if getattr(out, "_imd_gn_applied", False):
        r._imd_gn_applied = True
    st = getattr(out, "_imd_gn_stats", None)
    if st is not None:
        r._imd_gn_stats = st          # (a view is a new tensor object: carry the producer's GroupNorm statistics over)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# Upsample2D (nearest-2x interpolate -> 3x3 conv) as four 2x2 phase convolutions (csrc/conv_ups_phase.hip::conv_ups_phase_kernel;
# include/imagdressing_hip.h::imd_conv_ups_phase): after the upsample the four pixels of a 2x2 output block see the same 2x2 source
# pixels, so the 3x3 taps that fall on one source pixel are summed once per layer and four taps run instead of nine.  A/B switch,
# default on; IMD_UPS_PHASE=0 restores conv2d_nhwc(ups=True), whose dispatch is untouched.
# ---------------------------------------------------------------------------------------------------------------------
UPS_PHASE = _os.environ.get("IMD_UPS_PHASE", "1") != "0"
UPS_PHASE_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))      # [phase p][tap d] -> the 3x3 taps k that read source pixel y + p - 1 + d (the same in x)
UPS_PHASE_CFG = "ups_phase"                            # what the event hook records in place of a tile config
_UPS_W: Dict[Tuple, tuple] = {}
_UPS_OK: Dict[Tuple, bool] = {}
_clear_hooks.append(_UPS_W.clear)
_clear_hooks.append(_UPS_OK.clear)


def _pack_upsample_phase(w: torch.Tensor, dtype=None) -> torch.Tensor:
    N, Cp = w.shape[0], w.shape[1] // 9
    acc_dt = torch.float32 if w.dtype in DTYPE_CODE else w.dtype       # 16-bit weights: sum in fp32, round once
    w9 = w.to(acc_dt).view(N, 3, 3, Cp)
    out = torch.zeros(4, N, 4, Cp, dtype=acc_dt, device=w.device)
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    for ky in UPS_PHASE_TAPS[py][dy]:
                        for kx in UPS_PHASE_TAPS[px][dx]:
                            out[2 * py + px, :, 2 * dy + dx] += w9[:, ky, kx]
    return out.to(w.dtype if dtype is None else dtype).contiguous()


def pack_upsample_phase(w: torch.Tensor, dtype=None) -> torch.Tensor:
    """Phase weights of :func:`conv_ups_phase` [4 phases py*2+px][Cout][4 taps dy*2+dx][Cin_p] from the packed 3x3 weight ``w``
    [Cout, 9 * Cin_p] (tap-major: ky, kx, channel), in ``dtype`` (default: ``w``'s): summed in fp32, rounded once.  Packed from a 16-bit ``w`` the
    sums carry a second rounding; a caller that still holds the layer's fp32 weight can hand that in with ``dtype`` = the activation type.
    16/9 of the layer's weight bytes.
    Host-side, once per layer: cached against the storage and version of ``w`` (which the cache keeps alive) -- the first call
    must lie outside any HIP-graph capture (the pipelines run one step eagerly before they capture)."""
    if w.dim() != 2 or w.shape[1] % 9:
        raise L.ImdError(f"pack_upsample_phase: expected a packed 3x3 weight [Cout, 9 * Cin], got {tuple(w.shape)}")
    key = (w.data_ptr(), w._version, w.dtype, str(w.device), tuple(w.shape), dtype)
    ent = _UPS_W.get(key)
    if ent is None:
        if len(_UPS_W) > 64:
            _UPS_W.clear()
        ent = _UPS_W[key] = (w, _pack_upsample_phase(w, dtype))
    return ent[1]


def _ups_phase_block(shape, N: int, dtype):
    """The parameter block of the 9-tap problem conv3x3(nearest2x(x [B, H, W, Cin])) -> N channels (geometry only, no pointers)."""
    B, H, W, Cin = shape
    p = L.ConvGemmParams()
    p.flags = _gemm_call_flags()
    p.dtype, p.M, p.N, p.K, p.Cin, p.taps = DTYPE_CODE[dtype], 4 * B * H * W, N, 9 * Cin, Cin, 9
    p.Hin, p.Win, p.Hout, p.Wout, p.stride, p.ups = H, W, 2 * H, 2 * W, 1, 1
    p.x_pix_stride, p.out_ld, p.res_ld, p.out_scale, p.split_k = Cin, N, N, 1.0, 1
    return p


def conv_ups_phase_supported(x: torch.Tensor, w: torch.Tensor, bias=None) -> bool:
    """Should ``conv3x3(nearest2x(x)) + bias`` of ``x`` [B, H, W, Cin] with the packed 3x3 weight ``w`` [Cout, 9 * Cin] run as four phase convolutions
    (``imd_conv_ups_phase_supported``: Cin % 32 == 0, operands < 2 GiB, clearly fewer tile-padded multiplies than the 9-tap form, and a grid of at
    least 160 workgroups -- the smallest at which a gain over the K-sliced 9-tap launch has been measured)?
    A pure function of the geometry: remembered per geometry."""
    if x.dim() != 4 or w.dim() != 2 or w.shape[1] != 9 * x.shape[3] or x.dtype not in DTYPE_CODE or w.dtype != x.dtype or not x.is_contiguous():
        return False
    key = (tuple(x.shape), w.shape[0], x.dtype)
    ok = _UPS_OK.get(key)
    if ok is None:
        ok = bool(L.load().imd_conv_ups_phase_supported(C.byref(_ups_phase_block(x.shape, w.shape[0], x.dtype))))
        if len(_UPS_OK) < 4096:
            _UPS_OK[key] = ok
    return ok


def conv_ups_phase(x: torch.Tensor, w: torch.Tensor, bias=None, *, out: Optional[torch.Tensor] = None,
                   phase_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, H, W, Cin] 16-bit -> conv3x3(nearest2x(x), padding 1) + bias [B, 2H, 2W, Cout] in one launch of four taps per output pixel
    (include/imagdressing_hip.h::imd_conv_ups_phase).  ``w`` is the layer's packed 3x3 weight [Cout, 9 * Cin]; its phase form comes from
    :func:`pack_upsample_phase` (cached) unless the caller hands in ``phase_weights`` [4, Cout, 4, Cin] it packed itself.  Runs whatever the kernel
    computes correctly (Cin % 32 == 0, contiguous operands < 2 GiB) and raises otherwise -- there is no fallback in here; whether the launch PAYS
    is :func:`conv_ups_phase_supported`, which the call sites ask first.
    Counted and traced as the 9-tap convolution it computes (2 M N K with K = 9 Cin)."""
    ensure_device(x.device)
    B, H, W, Cin = x.shape
    N = w.shape[0]
    M, K = 4 * B * H * W, 9 * Cin
    dt = x.dtype
    if w.dim() != 2 or tuple(w.shape) != (N, K) or w.dtype != dt:
        raise L.ImdError(f"conv_ups_phase: expected a packed 3x3 weight [{N}, {K}] of {dt}, got {tuple(w.shape)} {w.dtype}")
    wp = pack_upsample_phase(w) if phase_weights is None else phase_weights
    if tuple(wp.shape) != (4, N, 4, Cin):
        raise L.ImdError(f"conv_ups_phase: phase weights must be [4, {N}, 4, {Cin}], got {tuple(wp.shape)}")
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, N), dtype=dt, device=x.device)
    elif out.numel() != M * N:
        raise L.ImdError(f"conv_ups_phase: out has {out.numel()} elements, expected {M * N}")
    p = _ups_phase_block(x.shape, N, dt)
    p.x, p.w, p.out = _dev(x, dt, "x"), _dev(wp, dt, "phase weights"), _dev(out, dt, "out")
    p.bias = None if bias is None else _dev(bias, torch.float32, "bias")
    _count("gemm_conv", 2.0 * M * N * K)
    if GEMM_TRACE is not None:
        GEMM_TRACE.append(dict(M=M, N=N, K=K, Cin=Cin, taps=9, Hin=H, Win=W, Hout=2 * H, Wout=2 * W, stride=1, ups=1, splittable=True, dtype=str(x.dtype),
                               bias=bias is not None, rowvec=False, rowvec_stride=0, res=False, res_rows=0, act=ACT_NONE, out_f32=False, heads=None,
                               gn_stats_groups=0, x_pix_stride=Cin, out_scale=1.0, pad_br_only=False, out_ld=N, res_ld=N, gn=False, gn_in=False, gn_out=False,
                               ups_phase=True))
    lib = L.load()
    if GEMM_EVENT_HOOK is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.imd_conv_ups_phase(C.byref(p), _stream()))
        e1.record()
        GEMM_EVENT_HOOK.setdefault((f"{M},{N},{K},9,1,1|{2 * H}x{2 * W}", UPS_PHASE_CFG, 1), []).append((e0, e1))
    else:
        L.check(lib.imd_conv_ups_phase(C.byref(p), _stream()))
    return out.view(B, 2 * H, 2 * W, N)


# bench.py installs {"match": fn(**shape) -> bool, "events": []} to bracket matching launches with HIP
# events on the launch stream (roofline measurement inside the timed region); None = no overhead.
ATTN_EVENT_HOOK = None


# the out-projection of the 64x64-level attention layers inside the attention launch (ABI v7, attention_d40.hip PROJ): the level-0
# hybrid block = two launches (norm1 + q/k/v, attention + out-projection + residual).  OPT-IN (IMD_FUSED_OUT_PROJ=1): correct and
# tested, but measured 7.5 % SLOWER end to end than the three-launch form (profiles/r3ao_*, r3ap_*)
FUSED_OUT_PROJ = _os.environ.get("IMD_FUSED_OUT_PROJ", "0") == "1"


def attention_proj_supported(H: int, N: int, D: int) -> bool:
    """Can imd_attention carry the block's out-projection (ABI v7)?  Head dim 40, 8 heads, N >= 512: the 64x64-level blocks."""
    return D == 40 and H * D == 320 and N >= 512


_proj_cnt: Dict[Tuple, torch.Tensor] = {}


def proj_counters(n: int, device) -> torch.Tensor:
    """Zeroed arrival counters of the fused out-projection (one per batch entry and 256-row block); every launch leaves them zero."""
    key = (str(device), _stream())
    t = _proj_cnt.get(key)
    if t is None or t.numel() < n:
        t = torch.zeros(max(n, 4096), dtype=torch.int32, device=device)
        _proj_cnt[key] = t
    return t


def attention_dup_supported(H: int, N: int, D: int) -> bool:
    """Can imd_attention also store the first-phase result to ``out_dup`` (ABI v9)?  Head dim 40, N >= 512: the 64x64-level blocks."""
    return bool(L.load().imd_attention_dup_supported(H, N, D))


# (round 6) phase-split launch of the hybrid attention at the 32x32 / 16x16 / 8x8 levels (imd_attn_params.phase2_rows; A/B switch)
ATTN_PHASE_SPLIT = _os.environ.get("IMD_ATTN_PHASE_SPLIT", "1") != "0"
ATTN_PHASE_SPLIT_MAX_N = int(_os.environ.get("IMD_ATTN_PHASE_SPLIT_MAX_N", "512"))      # (kernel alone, tools/attn_bench.py --phase-split: N = 256: 29.6 -> 19.8 us, N = 64: 15.5 -> 11.3 us, N = 1024: 60.3 -> 64.0 us)


@functools.lru_cache(maxsize=None)
def attention_phase_split_supported(D: int) -> bool:
    return bool(L.load().imd_attention_phase_split_supported(D))


def attention(q, k1, v1t, out, *, B, H, N, D, L1, L1P, kv1_bdiv=1, k2=None, v2t=None, scale2=None,
              L2=0, L2P=0, kv2_bdiv=1, out_ld=None, causal=False, k_pad_one=False, proj=None, out_dup=None, phase2_rows=0):
    """``k_pad_one``: k1 (and k2) came from :func:`k_buffer`, i.e. their pad column D holds 1.0 (see the header).
    ``phase2_rows`` = R: the caller guarantees that exactly the rows [0, R) have a non-zero ``scale2`` (the cond half of a CFG batch); where the library
    takes it (:func:`attention_phase_split_supported`, switch ``ATTN_PHASE_SPLIT``) the two softmaxes of those rows run as separate workgroups of ONE launch
    and a follow-up elementwise launch adds them -- bit-identical to the one-workgroup form, half as long per workgroup.  Ignored elsewhere.
    ``out_dup`` [B, N, C]: also receives softmax(Q K1^T) V1 of every batch entry (the paired uncond rows of a CFG batch's first hybrid
    block, :func:`attention_dup_supported`).
    ``proj`` = (w [C, C], bias [C] fp32 | None, residual [B, N, C] | None, proj_out [B, N, C]): the out-projection fused into the
    launch (:func:`attention_proj_supported`); returns proj_out then."""
    ensure_device(q.device)
    p = L.AttnParams()
    dt = q.dtype
    p.dtype = _code(q, "q")
    p.q, p.k1, p.v1t = _dev(q, dt, "q"), _dev(k1, dt, "k1"), _dev(v1t, dt, "v1t")
    p.k2, p.v2t = _opt(k2, dt, "k2"), _opt(v2t, dt, "v2t")
    p.scale2 = _opt(scale2, torch.float32, "scale2")
    p.out = _dev(out, dt, "out")
    p.B, p.H, p.N, p.D = B, H, N, D
    p.L1, p.L1P, p.kv1_bdiv = L1, L1P, kv1_bdiv
    p.L2, p.L2P, p.kv2_bdiv = L2, L2P, kv2_bdiv
    p.out_ld = H * D if out_ld is None else out_ld
    p.causal = int(causal)
    p.k_pad_one = int(bool(k_pad_one))
    p.flags = _attn_call_flags()
    if out_dup is not None:
        if out_dup.numel() != out.numel():
            raise L.ImdError("attention: out_dup must have the shape of out")
        p.out_dup = _dev(out_dup, dt, "out_dup")
    if phase2_rows and ATTN_PHASE_SPLIT and k2 is not None and scale2 is not None and proj is None and out_dup is None and not causal \
            and 0 < phase2_rows <= B and attention_phase_split_supported(D) and N <= ATTN_PHASE_SPLIT_MAX_N:
        p.phase2_rows = int(phase2_rows)
        p.phase2_out = workspace("attn_phase2", (phase2_rows * N * H * D,), torch.float32, q.device).data_ptr()
    ret = out
    if proj is not None:
        pw, pb, pres, pout = proj
        Cc = H * D
        if pw.numel() != Cc * Cc or pout.numel() != B * N * Cc or (pres is not None and pres.numel() != B * N * Cc):
            raise L.ImdError(f"attention: fused out-projection operands do not match B={B} N={N} C={Cc}")
        p.proj_w, p.proj_b = _dev(pw, dt, "proj_w"), _opt(pb, torch.float32, "proj_b")
        p.proj_res, p.proj_out = _opt(pres, dt, "proj_res"), _dev(pout, dt, "proj_out")
        p.proj_res_ld = p.proj_out_ld = Cc
        p.proj_counters = proj_counters(B * ((N + 255) // 256), q.device).data_ptr()
        ret = pout
        _count("gemm", 2.0 * B * N * Cc * Cc)
    if FLOP_COUNTER is not None:          # (reads scale2 back: counting mode only)
        rows2 = 0 if (k2 is None or scale2 is None) else int((scale2 != 0).sum().item())
        _count("attention", 4.0 * H * N * D * (B * L1 * (0.5 if causal else 1.0) + rows2 * L2))
    hook = ATTN_EVENT_HOOK
    if hook is not None and hook["match"](B=B, H=H, N=N, D=D, L1=L1, L2=L2 if k2 is not None else 0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.load().imd_attention(C.byref(p), _stream()))
        e1.record()
        hook["events"].append((e0, e1))
        return ret
    L.check(L.load().imd_attention(C.byref(p), _stream()))
    return ret


# ---------------------------------------------------------------------------------------------------------------------
# MX-FP8 attention (BASELINE.json configs[4]: "... with fp8 MFMA attention"): opt-in, head dim 40 (UNet level 0) only
# ---------------------------------------------------------------------------------------------------------------------
ATTN_FP8 = False                       # processors route d = 40 attention through imd_attention_fp8 when set
FP8_EXPS = dict(q=4, k=2, v=3)         # operands are stored as value * 2^e in e4m3 (range 2^-9 .. 448); eq + ek <= 8


def quantize_fp8_rows(x: torch.Tensor, exp: int, pad_val: float = 0.0) -> torch.Tensor:
    """Q or K [.., L, 48] 16-bit -> e4m3 bytes [.., L, 64] (columns 0..39 * 2^exp, columns 40 / 41 = pad_val)."""
    ensure_device(x.device)
    if x.shape[-1] != 48:
        raise L.ImdError(f"quantize_fp8_rows: expected head-dim-40 rows padded to 48, got {tuple(x.shape)}")
    rows = x.numel() // 48
    out = torch.empty(x.shape[:-1] + (64,), dtype=torch.uint8, device=x.device)
    L.check(L.load().imd_attn_quantize_fp8(_dev(x, x.dtype, "x"), out.data_ptr(), 0, rows, 0, exp, float(pad_val), _code(x, "x"), _stream()))
    return out


def quantize_fp8_vt(vt: torch.Tensor, exp: int) -> torch.Tensor:
    """V^T [.., 64, LP] 16-bit -> e4m3 bytes [.., 64, LP] (rows 0..39), keys permuted inside 64-groups as the kernel expects."""
    ensure_device(vt.device)
    if vt.shape[-2] != 64 or vt.shape[-1] % 64:
        raise L.ImdError(f"quantize_fp8_vt: expected [.., 64, LP] with LP % 64 == 0, got {tuple(vt.shape)}")
    LP = vt.shape[-1]
    groups = vt.numel() // (64 * LP)
    out = torch.zeros(vt.shape, dtype=torch.uint8, device=vt.device)
    L.check(L.load().imd_attn_quantize_fp8(_dev(vt, vt.dtype, "vt"), out.data_ptr(), 1, groups, LP, exp, 0.0, _code(vt, "vt"), _stream()))
    return out


def attention_fp8(q8, k1, v1t, out, *, B, H, N, L1, L1P, kv1_bdiv=1, k2=None, v2t=None, scale2=None, L2=0, L2P=0, kv2_bdiv=1,
                  out_ld=None, exps=None):
    """imd_attention_fp8 on e4m3 operands from quantize_fp8_rows / quantize_fp8_vt (head dim 40); ``out`` is 16-bit."""
    ensure_device(out.device)
    e = dict(FP8_EXPS, **(exps or {}))
    u8 = torch.uint8
    p = L.AttnParams()
    p.dtype = _code(out, "out")
    p.q, p.k1, p.v1t = _dev(q8, u8, "q8"), _dev(k1, u8, "k1"), _dev(v1t, u8, "v1t")
    p.k2, p.v2t = _opt(k2, u8, "k2"), _opt(v2t, u8, "v2t")
    p.scale2 = _opt(scale2, torch.float32, "scale2")
    p.out = _dev(out, out.dtype, "out")
    p.B, p.H, p.N, p.D = B, H, N, 40
    p.L1, p.L1P, p.kv1_bdiv = L1, L1P, kv1_bdiv
    p.L2, p.L2P, p.kv2_bdiv = L2, L2P, kv2_bdiv
    p.out_ld = H * 40 if out_ld is None else out_ld
    L.check(L.load().imd_attention_fp8(C.byref(p), e["q"], e["k"], e["v"], _stream()))
    return out


def group_norm(x: torch.Tensor, gamma, beta, *, groups=32, eps=1e-5, silu=False, out=None) -> torch.Tensor:
    """x [B, HW, C] (or [B, H, W, C]) bf16 NHWC."""
    ensure_device(x.device)
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    if out is None:
        out = torch.empty_like(x)
    lib = L.load()
    nws = lib.imd_groupnorm_workspace_floats(B, HW, Cc, groups)
    part = workspace("gn_partial", (max(nws, 1),), torch.float32, x.device)
    p = L.GroupNormParams()
    p.dtype = _code(x, "x")
    p.x, p.y = _dev(x, x.dtype, "x"), _dev(out, x.dtype, "out")
    p.gamma, p.beta = _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta")
    p.partial = part.data_ptr()
    p.B, p.HW, p.C, p.G, p.x_ld, p.y_ld = B, HW, Cc, groups, Cc, Cc
    p.eps, p.silu = eps, int(silu)
    st = getattr(x, "_imd_gn_stats", None)        # statistics written by the epilogue of the convolution that produced x
    if st is not None and st[2] == groups and st[0].shape[0] == B and FUSED_GN_STATS:
        p.partial, p.nparts = st[0].data_ptr(), st[1]
    L.check(lib.imd_groupnorm(C.byref(p), _stream()))
    return out


def group_norm_coeffs(x: torch.Tensor, gamma, beta, *, groups=32, eps=1e-5):
    """GroupNorm statistics of x [B, HW, C] as per-(batch, channel) fp32 (a, b) with y = x*a + b: the operand of
    conv_gemm's fused prologue (``gn=(a, b, silu)``)."""
    ensure_device(x.device)
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    lib = L.load()
    nws = lib.imd_groupnorm_workspace_floats(B, HW, Cc, groups)
    part = workspace("gn_partial", (max(nws, 1),), torch.float32, x.device)
    ab = torch.empty((2, B, Cc), dtype=torch.float32, device=x.device)
    p = L.GroupNormParams()
    p.dtype = _code(x, "x")
    p.x, p.y = _dev(x, x.dtype, "x"), None
    p.gamma, p.beta = _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta")
    p.partial = part.data_ptr()
    p.B, p.HW, p.C, p.G, p.x_ld, p.y_ld = B, HW, Cc, groups, Cc, Cc
    p.eps, p.silu = eps, 0
    st = getattr(x, "_imd_gn_stats", None)        # statistics written by the producer of x (see group_norm): no statistics pass
    if st is not None and st[2] == groups and st[0].shape[0] == B and FUSED_GN_STATS:
        p.partial, p.nparts = st[0].data_ptr(), st[1]
    L.check(lib.imd_groupnorm_coeffs(C.byref(p), ab[0].data_ptr(), ab[1].data_ptr(), _stream()))
    return ab[0], ab[1]


def lincomb(terms, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_j c_j * x_j over 1..8 (coefficient, fp32 tensor) pairs of equal numel; ``out`` may be one of the inputs."""
    xs = [t for _, t in terms]
    ensure_device(xs[0].device)
    n, numel = len(terms), xs[0].numel()
    for t in xs:
        if t.numel() != numel:
            raise L.ImdError("lincomb: all tensors must have the same number of elements")
    if out is None:
        out = torch.empty_like(xs[0])
    ptrs = (C.c_void_p * n)(*[_dev(t, torch.float32, "lincomb input") for t in xs])
    coefs = (C.c_float * n)(*[float(c) for c, _ in terms])
    L.check(L.load().imd_lincomb(ptrs, coefs, n, _dev(out, torch.float32, "out"), numel, _stream()))
    return out


def embed_tokens(table: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """table [V, C], pos [T, C] 16-bit, ids [B, T] int64 -> [B, T, C] = table[ids] + pos."""
    ensure_device(table.device)
    B, T = ids.shape
    V, Cc = table.shape
    out = torch.empty((B, T, Cc), dtype=table.dtype, device=table.device)
    L.check(L.load().imd_embed_tokens(_dev(table, table.dtype, "table"), V, _dev(pos, table.dtype, "pos"), pos.shape[0],
                                      _dev(ids, torch.int64, "ids"), out.data_ptr(), B * T, Cc, _code(table, "table"), _stream()))
    return out


def vit_assemble(patches: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """patches [B, P, C], cls [C], pos [P + 1, C] -> [B, P + 1, C] (class token first, position embeddings added)."""
    ensure_device(patches.device)
    B, P, Cc = patches.shape
    out = torch.empty((B, P + 1, Cc), dtype=patches.dtype, device=patches.device)
    L.check(L.load().imd_vit_assemble(_dev(patches, patches.dtype, "patches"), _dev(cls, patches.dtype, "cls"), _dev(pos, patches.dtype, "pos"),
                                      out.data_ptr(), B, P, Cc, _code(patches, "patches"), _stream()))
    return out


def softmax_rows(s: torch.Tensor, dtype=bf16, out=None) -> torch.Tensor:
    """Row softmax of an fp32 matrix [rows, cols] -> 16-bit probabilities (cols <= 16384).  ``out`` may have wider rows
    (only the first ``cols`` columns of each row are written)."""
    ensure_device(s.device)
    rows, cols = s.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=dtype, device=s.device)
    elif out.shape[0] != rows or out.shape[1] < cols:
        raise L.ImdError(f"softmax_rows: out {tuple(out.shape)} does not hold a [{rows}, {cols}] matrix")
    L.check(L.load().imd_softmax_rows(_dev(s, torch.float32, "s"), s.stride(0), _dev(out, out.dtype, "out"), out.stride(0),
                                      rows, cols, _code(out, "out"), _stream()))
    return out


def layer_norm(x: torch.Tensor, gamma, beta, eps=1e-5, out=None) -> torch.Tensor:
    ensure_device(x.device)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    if out is None:
        out = torch.empty_like(x)
    p = L.LayerNormParams()
    p.dtype = _code(x, "x")
    p.x, p.y = _dev(x, x.dtype, "x"), _dev(out, x.dtype, "out")
    p.gamma, p.beta = _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta")
    p.rows, p.C, p.x_ld, p.y_ld, p.eps = rows, Cc, Cc, Cc, eps
    L.check(L.load().imd_layernorm(C.byref(p), _stream()))
    return out


def ddim_coefs(a_t, a_prev, a_next=None):
    """The six schedule coefficients of one DDIM step in the order imd_ddim_params.coefs reads them."""
    an = (1.0, 0.0) if a_next is None else (a_next ** 0.5, (1 - a_next) ** 0.5)
    return [a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, (1 - a_prev) ** 0.5, an[0], an[1]]


def ddim_cfg_step(z, eps, x_next, *, guidance, a_t=1.0, a_prev=1.0, mask=None, z_img=None, noise=None, a_next=None, coefs=None,
                  var_noise=None, sigma=0.0):
    """z [B,HW,4] fp32 (in place); eps [2B,HW,4] fp32; x_next [2B,HW,8] bf16 or None.  ``coefs``: device fp32 [6]
    (:func:`ddim_coefs`) read by the kernel instead of a_t / a_prev / a_next (HIP-graph replay of a step).
    ``var_noise`` [B,HW,4] fp32 + ``sigma``: the stochastic DDIM step (eta > 0) -- diffusers' ``DDIMScheduler.step``:
    direction coefficient sqrt(1 - a_prev - sigma^2), ``+ sigma * var_noise``.
    ``guidance``: a float (``imd_ddim_cfg_step``), or a device fp32 tensor [B] -- the scale of each latent row
    (``imd_ddim_cfg_step_rows``: a batch of requests with different guidance scales)."""
    ensure_device(z.device)
    B, HW = z.shape[0], z.shape[1]
    rows = None
    if isinstance(guidance, torch.Tensor):
        if guidance.dtype != torch.float32 or guidance.numel() != B or not guidance.is_contiguous():
            raise L.ImdError(f"ddim_cfg_step: per-row guidance must be a contiguous fp32 tensor of {B} values, got "
                             f"{guidance.dtype} {tuple(guidance.shape)}")
        rows = _dev(guidance, torch.float32, "guidance")
        guidance = 0.0                           # (ignored by the per-row entry point)
    p = L.DdimParams()
    p.z, p.eps = _dev(z, torch.float32, "z"), _dev(eps, torch.float32, "eps")
    p.dtype = 0 if x_next is None else _code(x_next, "x_next")
    p.x_next = None if x_next is None else _dev(x_next, x_next.dtype, "x_next")
    p.B, p.HW = B, HW
    p.guidance = guidance
    p.sqrt_a_t, p.sqrt_1m_a_t = a_t ** 0.5, (1 - a_t) ** 0.5
    p.sqrt_a_prev, p.sqrt_1m_a_prev = a_prev ** 0.5, (1 - a_prev) ** 0.5
    p.var_noise, p.sigma = None, 0.0
    if var_noise is not None:
        if var_noise.numel() != B * HW * 4:
            raise L.ImdError(f"ddim_cfg_step: var_noise has {var_noise.numel()} elements, expected {B * HW * 4}")
        p.var_noise, p.sigma = _dev(var_noise, torch.float32, "var_noise"), float(sigma)
        p.sqrt_1m_a_prev = max(1 - a_prev - float(sigma) ** 2, 0.0) ** 0.5
    p.mask = _opt(mask, torch.float32, "mask")
    p.z_img = _opt(z_img, torch.float32, "z_img")
    p.noise = _opt(noise, torch.float32, "noise")
    if a_next is None:
        p.sqrt_a_next, p.sqrt_1m_a_next = 1.0, 0.0
    else:
        p.sqrt_a_next, p.sqrt_1m_a_next = a_next ** 0.5, (1 - a_next) ** 0.5
    p.coefs = _opt(coefs, torch.float32, "coefs")
    if coefs is not None and coefs.numel() < 6:
        raise L.ImdError("ddim_cfg_step: coefs needs 6 fp32 values")
    if rows is None:
        L.check(L.load().imd_ddim_cfg_step(C.byref(p), _stream()))
    else:
        L.check(L.load().imd_ddim_cfg_step_rows(C.byref(p), rows, _stream()))
    return z


SAMPLER_MAX_HISTORY = 4
SAMPLER_COEFS = 13


def sampler_coefs(m_x=0.0, m_e=1.0, z_x=1.0, z_m=0.0, z_h=(), z_n=0.0, b_img=1.0, b_noise=0.0, in_scale=1.0, store=-1):
    """The coefficient block of one ``imd_sampler_step`` in the order ``imd_sampler_params.coefs`` reads it (13 floats; ``z_h`` by
    PHYSICAL history slot, padded with zeros; ``store`` = the slot that receives m, -1 for none, carried as a float)."""
    zh = [float(c) for c in z_h]
    if len(zh) > SAMPLER_MAX_HISTORY:
        raise L.ImdError(f"sampler_coefs: {len(zh)} history coefficients (at most {SAMPLER_MAX_HISTORY})")
    zh += [0.0] * (SAMPLER_MAX_HISTORY - len(zh))
    return [float(m_x), float(m_e), float(z_x), float(z_m)] + zh + [float(z_n), float(b_img), float(b_noise), float(in_scale), float(int(store))]


def _sampler_params(what, z, eps, x_next, guidance, hist, noise, mask, z_img, blend_noise, rows=None, unipc=False):
    """the tensor fields of ``imd_sampler_params`` (everything but the coefficients), checked: shared by the entry points.  ``rows``:
    the batch width B of ``imd_sampler_step_rows_at``, whose z / hist / noise / blend operands have ``z.shape[0]`` = slots rows while
    eps, x_next and the guidance array have B; None: one row count for everything.  ``unipc``: the same fields of
    ``imd_unipc_params`` (which has no ``noise``)."""
    ensure_device(z.device)
    S, HW = z.shape[0], z.shape[1]
    B = S if rows is None else int(rows)
    n, nr = S * HW * 4, B * HW * 4
    p = L.UnipcParams() if unipc else L.SamplerParams()
    p.z, p.eps = _dev(z, torch.float32, "z"), _dev(eps, torch.float32, "eps")
    if z.numel() != n or eps.numel() != 2 * nr:
        raise L.ImdError(f"{what}: z {tuple(z.shape)} / eps {tuple(eps.shape)}: expected [B, HW, 4] and [2B, HW, 4]" if rows is None else
                         f"{what}: z {tuple(z.shape)} / eps {tuple(eps.shape)}: expected [slots, HW, 4] and [2 x {B}, HW, 4]")
    p.dtype = 0 if x_next is None else _code(x_next, "x_next")
    p.x_next = None if x_next is None else _dev(x_next, x_next.dtype, "x_next")
    if x_next is not None and x_next.numel() != 4 * nr:
        raise L.ImdError(f"{what}: x_next has {x_next.numel()} elements, expected {4 * nr}")
    p.B, p.HW = B, HW
    if isinstance(guidance, torch.Tensor):
        if guidance.dtype != torch.float32 or guidance.numel() != B or not guidance.is_contiguous():
            raise L.ImdError(f"{what}: per-row guidance must be a contiguous fp32 tensor of {B} values, got "
                             f"{guidance.dtype} {tuple(guidance.shape)}")
        p.guidance_rows, p.guidance = _dev(guidance, torch.float32, "guidance"), 0.0
    else:
        p.guidance_rows, p.guidance = None, float(guidance)
    p.K, p.hist = 0, None
    if hist is not None:
        if hist.numel() % n:
            raise L.ImdError(f"{what}: hist has {hist.numel()} elements, not a multiple of {n}")
        p.K, p.hist = hist.numel() // n, _dev(hist, torch.float32, "hist")
    for name, t in (("noise", noise), ("z_img", z_img), ("blend_noise", blend_noise)):
        if t is not None and t.numel() != n:
            raise L.ImdError(f"{what}: {name} has {t.numel()} elements, expected {n}")
    if mask is not None and mask.numel() != S * HW:
        raise L.ImdError(f"{what}: mask has {mask.numel()} elements, expected {S * HW}")
    p.mask, p.z_img, p.blend_noise = _opt(mask, torch.float32, "mask"), _opt(z_img, torch.float32, "z_img"), _opt(blend_noise, torch.float32, "blend_noise")
    p.coefs = None
    if unipc:
        p.store_m = p.store_s = -1
    else:
        p.noise, p.store = _opt(noise, torch.float32, "noise"), -1
    return p


def sampler_step(z, eps, x_next, *, guidance, coefs, hist=None, noise=None, mask=None, z_img=None, blend_noise=None):
    """One fused step of an affine sampler (``imd_sampler_step``; DPM-Solver++, Euler, Euler-ancestral, PNDM -- the coefficients
    come from imagdressing_amd/scheduler.py).  z [B,HW,4] fp32 (in place); eps [2B,HW,4] fp32; x_next [2B,HW,8] 16-bit or None;
    ``hist`` [K, B, HW, 4] fp32 (one contiguous buffer, K <= 4) or None; ``noise`` [B,HW,4] fp32 (scaled by z_n);
    ``mask`` [B,HW] + ``z_img`` + ``blend_noise`` [B,HW,4]: the inpainting blend.
    ``coefs``: the 13 values of :func:`sampler_coefs` as a Python sequence (passed in the parameter block) or as a device fp32
    tensor (read by the kernel: HIP-graph replay of a step).  ``guidance``: a float, or a device fp32 tensor [B]."""
    p = _sampler_params("sampler_step", z, eps, x_next, guidance, hist, noise, mask, z_img, blend_noise)
    if isinstance(coefs, torch.Tensor):
        if coefs.numel() < SAMPLER_COEFS:
            raise L.ImdError(f"sampler_step: coefs needs {SAMPLER_COEFS} fp32 values")
        p.coefs = _dev(coefs, torch.float32, "coefs")
    else:
        c = [float(v) for v in coefs]
        if len(c) != SAMPLER_COEFS:
            raise L.ImdError(f"sampler_step: coefs needs {SAMPLER_COEFS} values (ops.sampler_coefs), got {len(c)}")
        p.m_x, p.m_e, p.z_x, p.z_m = c[0:4]
        p.z_h = (C.c_float * 4)(*c[4:8])
        p.z_n, p.b_img, p.b_noise, p.in_scale = c[8:12]
        p.store = int(c[12])
    L.check(L.load().imd_sampler_step(C.byref(p), _stream()))
    return z


SAMPLER_ROW_FLOATS = 16


def sampler_coef_row(coefs13, active=True):
    """One latent row of ``imd_sampler_step_rows``: the 13 values of :func:`sampler_coefs`, the ``active`` flag (0: the row is
    skipped, nothing of it is read or written) and two reserved zeros -- 16 floats."""
    c = [float(v) for v in coefs13]
    if len(c) != SAMPLER_COEFS:
        raise L.ImdError(f"sampler_coef_row: needs the {SAMPLER_COEFS} values of ops.sampler_coefs, got {len(c)}")
    return c + [1.0 if active else 0.0, 0.0, 0.0]


def sampler_step_rows(z, eps, x_next, *, guidance, coef_rows, hist=None, noise=None, mask=None, z_img=None, blend_noise=None):
    """:func:`sampler_step` with one coefficient block PER LATENT ROW (``imd_sampler_step_rows``): ``coef_rows`` is a device fp32
    tensor [B, 16] of :func:`sampler_coef_row` rows -- every row at its own step of its own schedule, with its own history slots; an
    inactive row keeps every byte of its z, history and x_next.  The other arguments as for :func:`sampler_step`."""
    p = _sampler_params("sampler_step_rows", z, eps, x_next, guidance, hist, noise, mask, z_img, blend_noise)
    if (not isinstance(coef_rows, torch.Tensor) or coef_rows.dtype != torch.float32 or coef_rows.numel() != p.B * SAMPLER_ROW_FLOATS
            or not coef_rows.is_contiguous()):
        raise L.ImdError(f"sampler_step_rows: coef_rows must be a contiguous device fp32 tensor [{p.B}, {SAMPLER_ROW_FLOATS}] "
                         f"(ops.sampler_coef_row per latent row), got {getattr(coef_rows, 'dtype', type(coef_rows))} "
                         f"{tuple(getattr(coef_rows, 'shape', ()))}")
    L.check(L.load().imd_sampler_step_rows(C.byref(p), _dev(coef_rows, torch.float32, "coef_rows"), _stream()))
    return z


def _coef_rows_ptr(what, coef_rows, B):
    if (not isinstance(coef_rows, torch.Tensor) or coef_rows.dtype != torch.float32 or coef_rows.numel() != B * SAMPLER_ROW_FLOATS
            or not coef_rows.is_contiguous()):
        raise L.ImdError(f"{what}: coef_rows must be a contiguous device fp32 tensor [{B}, {SAMPLER_ROW_FLOATS}] "
                         f"(ops.sampler_coef_row per row), got {getattr(coef_rows, 'dtype', type(coef_rows))} "
                         f"{tuple(getattr(coef_rows, 'shape', ()))}")
    return _dev(coef_rows, torch.float32, "coef_rows")


def _row_slot_ptr(what, row_slot, slots):
    """the device int32 map row -> slot of a compacting session; its length is the batch width B <= slots"""
    if (not isinstance(row_slot, torch.Tensor) or row_slot.dtype != torch.int32 or row_slot.dim() != 1 or not row_slot.is_contiguous()
            or not 1 <= row_slot.numel() <= slots):
        raise L.ImdError(f"{what}: row_slot must be a contiguous device int32 tensor [B] with 1 <= B <= slots = {slots}, got "
                         f"{getattr(row_slot, 'dtype', type(row_slot))} {tuple(getattr(row_slot, 'shape', ()))}")
    return _dev(row_slot, torch.int32, "row_slot")


def sampler_step_rows_at(z, eps, x_next, *, guidance, coef_rows, row_slot, hist=None, noise=None, mask=None, z_img=None, blend_noise=None):
    """:func:`sampler_step_rows` through a row -> slot map (``imd_sampler_step_rows_at``; the compacting denoising session).
    ``row_slot`` [B] int32 on the device: batch row r carries the request of slot ``row_slot[r]`` (-1, or anything outside
    0..slots-1: an idle row, skipped whole).  By ROW: ``eps`` [2B,HW,4], ``x_next`` [2B,HW,8], ``coef_rows`` [B,16], a ``guidance``
    tensor [B].  By SLOT: ``z`` [slots,HW,4] (in place), ``hist`` [K,slots,HW,4], ``noise``, ``mask`` / ``z_img`` / ``blend_noise``."""
    slots = z.shape[0]
    rs = _row_slot_ptr("sampler_step_rows_at", row_slot, slots)
    B = row_slot.numel()
    p = _sampler_params("sampler_step_rows_at", z, eps, x_next, guidance, hist, noise, mask, z_img, blend_noise, rows=B)
    L.check(L.load().imd_sampler_step_rows_at(C.byref(p), _coef_rows_ptr("sampler_step_rows_at", coef_rows, B), rs, slots, _stream()))
    return z


def session_input_rows(z, row_slot, in_scale_rows, x_in):
    """``x_in[r] = x_in[B + r] = 16-bit(in_scale_rows[r] * z[row_slot[r]])``, channels 4..7 zero (``imd_session_input_rows``): the
    UNet input of a session's batch rows from the fp32 latents, with the pack expression of the step's ``x_next``.  z [slots,HW,4]
    fp32; ``row_slot`` [B] int32 and ``in_scale_rows`` [B] fp32 on the device; ``x_in`` [2B,HW,8] 16-bit.  Rows whose slot is outside
    0..slots-1 keep their bytes."""
    ensure_device(z.device)
    if z.dim() != 3 or z.shape[2] != 4:
        raise L.ImdError(f"session_input_rows: z {tuple(z.shape)}: expected [slots, HW, 4]")
    slots, HW = z.shape[0], z.shape[1]
    zp = _dev(z, torch.float32, "z")
    rs = _row_slot_ptr("session_input_rows", row_slot, slots)
    B = row_slot.numel()
    if not isinstance(in_scale_rows, torch.Tensor) or in_scale_rows.numel() != B:
        raise L.ImdError(f"session_input_rows: in_scale_rows must be a device fp32 tensor of {B} values")
    if not isinstance(x_in, torch.Tensor) or x_in.numel() != 2 * B * HW * 8:
        raise L.ImdError(f"session_input_rows: x_in has {getattr(x_in, 'numel', lambda: 0)()} elements, expected {2 * B * HW * 8} ([2 x {B}, {HW}, 8])")
    L.check(L.load().imd_session_input_rows(zp, rs, _dev(in_scale_rows, torch.float32, "in_scale_rows"), _dev(x_in, x_in.dtype, "x_in"),
                                            B, slots, HW, _code(x_in, "x_in"), _stream()))
    return x_in


# ---- per-row LoRA scales: the augmented activation rows [x | s_row (x D^T)] (csrc/lora_rows.hip) ----
LORA_ROWS_COUNTER = {"launches": 0}      # imd_lora_expand_rows launches of this process (tests check that the folded route makes none)


def _rows2d(t, name: str):
    """(pointer, leading dimension) of a 16-bit [rows, cols] tensor or row-strided view of one"""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_cuda or t.dtype not in DTYPE_CODE or (t.shape[1] > 1 and t.stride(1) != 1):
        raise L.ImdError(f"lora_expand_rows: {name} must be a 16-bit [rows, channels] device tensor with contiguous channels")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def lora_expand_rows(x: torch.Tensor, down: torch.Tensor, row_scale: torch.Tensor, rows_per_entry: int, *,
                     out: Optional[torch.Tensor] = None, out_cols: Optional[int] = None) -> torch.Tensor:
    """``out[m, :C] = x[m]`` (the same bits), ``out[m, C + j] = 16-bit(row_scale[m // rows_per_entry] * sum_c x[m, c] down[j, c])``
    (``imd_lora_expand_rows``): the activations of a LoRA layer whose scale differs per row, for the projection launch with the augmented
    weight ``[W | U]``.  x [M, C] (rows may be strided), down [T, C] contiguous, row_scale fp32 [E] on the device with
    ``M == E * rows_per_entry``.  ``out``: a [M, >= C + T] tensor or row-strided view (columns past C + T keep their bytes); without it a
    fresh [M, out_cols or C + T] tensor whose columns past C + T are zero."""
    ensure_device(x.device)
    xp, x_ld = _rows2d(x, "x")
    M, C_ = x.shape
    if not isinstance(down, torch.Tensor) or down.dim() != 2 or down.shape[1] != C_ or down.dtype != x.dtype:
        raise L.ImdError(f"lora_expand_rows: down must be [T, {C_}] of {x.dtype}")
    T = down.shape[0]
    if not isinstance(row_scale, torch.Tensor) or row_scale.dim() != 1:
        raise L.ImdError("lora_expand_rows: row_scale must be a 1-d fp32 device tensor")
    if out is None:
        cols = C_ + T if out_cols is None else int(out_cols)
        out = torch.empty((M, cols), dtype=x.dtype, device=x.device) if cols == C_ + T else torch.zeros((M, cols), dtype=x.dtype, device=x.device)
    if out.dtype != x.dtype or out.shape[0] != M:
        raise L.ImdError(f"lora_expand_rows: out must be [{M}, >= {C_ + T}] of {x.dtype}")
    op, out_ld = _rows2d(out, "out")
    if out.shape[1] < C_ + T:
        raise L.ImdError(f"lora_expand_rows: out has {out.shape[1]} columns, needs {C_ + T}")
    p = L.LoraRowsParams()
    p.x, p.down, p.row_scale, p.out = xp, _dev(down, x.dtype, "down"), _dev(row_scale, torch.float32, "row_scale"), op
    p.M, p.C, p.T, p.E, p.rows_per_entry = M, C_, T, row_scale.numel(), int(rows_per_entry)
    p.x_ld, p.out_ld, p.dtype = x_ld, out_ld, _code(x, "x")
    L.check(L.load().imd_lora_expand_rows(C.byref(p), _stream()))
    LORA_ROWS_COUNTER["launches"] += 1
    _count("lora_expand", 2.0 * M * T * C_)
    return out


# ---- a scale per batch row on several tensors at once: the ControlNet residuals (csrc/residual_scale_rows.hip) ----
SCALE_ROWS_COUNTER = {"launches": 0}      # imd_residual_scale_rows launches of this process (tests check that the folded route makes none)
SCALE_ROWS_MAX_SEGMENTS = L.SCALE_ROWS_MAX_SEGMENTS


def residual_scale_rows(tensors: Sequence[torch.Tensor], scale_rows: torch.Tensor):
    """Row r of every tensor times ``scale_rows[r]``, in place, in one launch (``imd_residual_scale_rows``): 1 to 16 contiguous 16-bit
    device tensors of one dtype with equal ``shape[0]`` = rows whose rows hold a multiple of 8 elements, ``scale_rows`` fp32 [rows] on the
    device.  A row at exactly 1.0 keeps its bytes; every other gets ``(x.float() * s).to(dtype)``, round to nearest even."""
    what = "residual_scale_rows"
    if not isinstance(tensors, (list, tuple)) or not 1 <= len(tensors) <= SCALE_ROWS_MAX_SEGMENTS:
        n = len(tensors) if isinstance(tensors, (list, tuple)) else type(tensors).__name__
        raise L.ImdError(f"{what}: expected a list of 1 to {SCALE_ROWS_MAX_SEGMENTS} tensors, got {n}")
    if not all(isinstance(t, torch.Tensor) and t.dim() >= 1 for t in tensors):
        raise L.ImdError(f"{what}: every segment must be a torch.Tensor [rows, ...]")
    first = tensors[0]
    rows = first.shape[0]
    if any(t.shape[0] != rows for t in tensors):
        raise L.ImdError(f"{what}: the tensors differ in shape[0] ({[t.shape[0] for t in tensors]}): one scale per row of all of them")
    if any(t.dtype != first.dtype for t in tensors):
        raise L.ImdError(f"{what}: the tensors differ in dtype ({sorted({str(t.dtype) for t in tensors})})")
    if not isinstance(scale_rows, torch.Tensor) or scale_rows.dim() != 1 or scale_rows.numel() != rows:
        raise L.ImdError(f"{what}: scale_rows must be a 1-d fp32 device tensor of {rows} values, got "
                         f"{tuple(getattr(scale_rows, 'shape', ()))}")
    p = L.ScaleRowsParams()
    p.dtype, p.rows, p.segments = _code(first, what), rows, len(tensors)
    for k, t in enumerate(tensors):
        if rows < 1 or t.numel() == 0 or (t.numel() // rows) % 8:
            raise L.ImdError(f"{what}: tensor {k} {tuple(t.shape)}: a row must hold a positive multiple of 8 elements")
        if not t.is_contiguous():
            raise L.ImdError(f"{what}: tensor {k} must be contiguous (a segment is one [rows, row_elems] block)")
    for k, t in enumerate(tensors):
        p.data[k] = _dev(t, first.dtype, f"tensor {k}")
        p.row_elems[k] = t.numel() // rows
    ensure_device(first.device)
    p.scale_rows = _dev(scale_rows, torch.float32, "scale_rows")
    L.check(L.load().imd_residual_scale_rows(C.byref(p), _stream()))
    SCALE_ROWS_COUNTER["launches"] += 1
    return tensors


# ---- the scaled sum of several sources, a scale per source and batch row: several ControlNets' residuals (csrc/residual_mix_rows.hip) ----
MIX_ROWS_COUNTER = {"launches": 0}        # imd_residual_mix_rows launches of this process (tests check that one net makes none)
MIX_ROWS_MAX_SOURCES = L.MIX_ROWS_MAX_SOURCES
MIX_ROWS_MAX_SEGMENTS = L.MIX_ROWS_MAX_SEGMENTS


def residual_mix_rows(sources: Sequence[Sequence[torch.Tensor]], scales: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None):
    """``out[j][r] = 16-bit(sum over k of sources[k][j][r].float() * scales[k, r])`` in one launch (``imd_residual_mix_rows``): 1 to 4
    sources, each a list of the same 1 to 16 contiguous 16-bit device tensors [rows, ...] whose rows hold a multiple of 8 elements;
    ``scales`` fp32 [sources, rows] on the device.  The sum runs in source order in fp32, every product and every sum rounded (no FMA);
    a source whose scale for a row is 0 is not read there; all 0 gives +0.  ``out``: None (fresh tensors) or a list like one source,
    which may BE one of the sources (in place).  -> ``out``."""
    what = "residual_mix_rows"
    if not isinstance(sources, (list, tuple)) or not 1 <= len(sources) <= MIX_ROWS_MAX_SOURCES:
        n = len(sources) if isinstance(sources, (list, tuple)) else type(sources).__name__
        raise L.ImdError(f"{what}: expected a list of 1 to {MIX_ROWS_MAX_SOURCES} sources, got {n}")
    for k, src in enumerate(sources):
        if not isinstance(src, (list, tuple)) or not 1 <= len(src) <= MIX_ROWS_MAX_SEGMENTS:
            n = len(src) if isinstance(src, (list, tuple)) else type(src).__name__
            raise L.ImdError(f"{what}: source {k}: expected a list of 1 to {MIX_ROWS_MAX_SEGMENTS} tensors, got {n}")
        if not all(isinstance(t, torch.Tensor) and t.dim() >= 1 for t in src):
            raise L.ImdError(f"{what}: source {k}: every segment must be a torch.Tensor [rows, ...]")
    first = sources[0][0]
    rows, K, S = first.shape[0], len(sources), len(sources[0])
    if out is None:
        out = [torch.empty_like(t) for t in sources[0]]
    elif not isinstance(out, (list, tuple)) or not all(isinstance(t, torch.Tensor) for t in out):
        raise L.ImdError(f"{what}: out must be None or a list of tensors like one source")
    groups = [(f"source {k}", src) for k, src in enumerate(sources)] + [("out", out)]
    for name, g in groups:
        if len(g) != S:
            raise L.ImdError(f"{what}: {name} has {len(g)} segments, source 0 has {S}")
        for j, t in enumerate(g):
            if t.dtype != first.dtype:
                raise L.ImdError(f"{what}: {name}, tensor {j}: the tensors differ in dtype ({t.dtype} and {first.dtype})")
            if tuple(t.shape) != tuple(sources[0][j].shape):
                raise L.ImdError(f"{what}: {name}, tensor {j}: shape {tuple(t.shape)} differs from source 0's {tuple(sources[0][j].shape)}")
            if not t.is_contiguous():
                raise L.ImdError(f"{what}: {name}, tensor {j} must be contiguous (a segment is one [rows, row_elems] block)")
    if not isinstance(scales, torch.Tensor) or tuple(scales.shape) != (K, rows):
        raise L.ImdError(f"{what}: scales must be an fp32 device tensor [{K}, {rows}] (sources x rows), got "
                         f"{tuple(getattr(scales, 'shape', ()))}")
    p = L.MixRowsParams()
    p.dtype, p.rows, p.segments, p.sources = _code(first, what), rows, S, K
    for j, t in enumerate(sources[0]):
        if rows < 1 or t.numel() == 0 or (t.numel() // rows) % 8:
            raise L.ImdError(f"{what}: tensor {j} {tuple(t.shape)}: a row must hold a positive multiple of 8 elements")
        p.row_elems[j] = t.numel() // rows
    for k, src in enumerate(sources):
        for j, t in enumerate(src):
            p.src[k][j] = _dev(t, first.dtype, f"source {k}, tensor {j}")
    for j, t in enumerate(out):
        p.dst[j] = _dev(t, first.dtype, f"out, tensor {j}")
    ensure_device(first.device)
    p.scales = _dev(scales, torch.float32, "scales")
    L.check(L.load().imd_residual_mix_rows(C.byref(p), _stream()))
    MIX_ROWS_COUNTER["launches"] += 1
    return list(out)


# ---- UniPC on one fused step launch (csrc/unipc_step.hip;the coefficients come from scheduler.UniPCMultistepScheduler.plan_fused) ----
UNIPC_COEFS = 19
UNIPC_ROW_FLOATS = 24
UNIPC_IN_SCALE = 16          # index of in_scale in the block (what ``session_input_rows`` needs of a request's last step)


def unipc_coefs(m_x=0.0, m_e=1.0, s_x=1.0, s_m=0.0, s_h=(), z_s=1.0, z_m=0.0, z_h=(), b_img=1.0, b_noise=0.0, in_scale=1.0,
                store_m=-1, store_s=-1):
    """The coefficient block of one ``imd_unipc_step`` in the order ``imd_unipc_params.coefs`` reads it (19 floats; ``s_h`` / ``z_h`` by
    PHYSICAL history slot, padded with zeros; ``store_m`` / ``store_s`` = the slots that receive m and s', -1 for none, carried as
    floats)."""
    sh, zh = [float(c) for c in s_h], [float(c) for c in z_h]
    if len(sh) > SAMPLER_MAX_HISTORY or len(zh) > SAMPLER_MAX_HISTORY:
        raise L.ImdError(f"unipc_coefs: {max(len(sh), len(zh))} history coefficients (at most {SAMPLER_MAX_HISTORY})")
    sh += [0.0] * (SAMPLER_MAX_HISTORY - len(sh))
    zh += [0.0] * (SAMPLER_MAX_HISTORY - len(zh))
    return ([float(m_x), float(m_e), float(s_x), float(s_m)] + sh + [float(z_s), float(z_m)] + zh
            + [float(b_img), float(b_noise), float(in_scale), float(int(store_m)), float(int(store_s))])


def unipc_step(z, eps, x_next, *, guidance, coefs, hist=None, mask=None, z_img=None, blend_noise=None):
    """One fused UniPC step (``imd_unipc_step``): x0 prediction with CFG, corrector, predictor, both history stores, the inpainting
    blend and the next UNet input.  z [B,HW,4] fp32 (in place); eps [2B,HW,4] fp32; x_next [2B,HW,8] 16-bit or None; ``hist``
    [K, B, HW, 4] fp32 (one contiguous buffer, K = solver_order + 1 <= 4) or None; ``mask`` [B,HW] + ``z_img`` + ``blend_noise``
    [B,HW,4]: the inpainting blend.  ``coefs``: the 19 values of :func:`unipc_coefs` as a Python sequence (passed in the parameter
    block) or as a device fp32 tensor (read by the kernel: HIP-graph replay of a step).  ``guidance``: a float, or a device fp32
    tensor [B]."""
    p = _sampler_params("unipc_step", z, eps, x_next, guidance, hist, None, mask, z_img, blend_noise, unipc=True)
    if isinstance(coefs, torch.Tensor):
        if coefs.numel() < UNIPC_COEFS:
            raise L.ImdError(f"unipc_step: coefs needs {UNIPC_COEFS} fp32 values")
        p.coefs = _dev(coefs, torch.float32, "coefs")
    else:
        c = [float(v) for v in coefs]
        if len(c) != UNIPC_COEFS:
            raise L.ImdError(f"unipc_step: coefs needs {UNIPC_COEFS} values (ops.unipc_coefs), got {len(c)}")
        p.m_x, p.m_e, p.s_x, p.s_m = c[0:4]
        p.s_h = (C.c_float * 4)(*c[4:8])
        p.z_s, p.z_m = c[8:10]
        p.z_h = (C.c_float * 4)(*c[10:14])
        p.b_img, p.b_noise, p.in_scale = c[14:17]
        p.store_m, p.store_s = int(c[17]), int(c[18])
    L.check(L.load().imd_unipc_step(C.byref(p), _stream()))
    return z


def unipc_coef_row(coefs19, active=True):
    """One latent row of ``imd_unipc_step_rows``: the 19 values of :func:`unipc_coefs`, the ``active`` flag (0: the row is skipped,
    nothing of it is read or written) and four reserved zeros -- 24 floats."""
    c = [float(v) for v in coefs19]
    if len(c) != UNIPC_COEFS:
        raise L.ImdError(f"unipc_coef_row: needs the {UNIPC_COEFS} values of ops.unipc_coefs, got {len(c)}")
    return c + [1.0 if active else 0.0, 0.0, 0.0, 0.0, 0.0]


def _unipc_rows_ptr(what, coef_rows, B):
    if (not isinstance(coef_rows, torch.Tensor) or coef_rows.dtype != torch.float32 or coef_rows.numel() != B * UNIPC_ROW_FLOATS
            or not coef_rows.is_contiguous()):
        raise L.ImdError(f"{what}: coef_rows must be a contiguous device fp32 tensor [{B}, {UNIPC_ROW_FLOATS}] "
                         f"(ops.unipc_coef_row per row), got {getattr(coef_rows, 'dtype', type(coef_rows))} "
                         f"{tuple(getattr(coef_rows, 'shape', ()))}")
    return _dev(coef_rows, torch.float32, "coef_rows")


def unipc_step_rows(z, eps, x_next, *, guidance, coef_rows, hist=None, mask=None, z_img=None, blend_noise=None):
    """:func:`unipc_step` with one coefficient block PER LATENT ROW (``imd_unipc_step_rows``): ``coef_rows`` is a device fp32 tensor
    [B, 24] of :func:`unipc_coef_row` rows -- every row at its own step of its own schedule, with its own history slots; an inactive
    row keeps every byte of its z, history and x_next.  The other arguments as for :func:`unipc_step`."""
    p = _sampler_params("unipc_step_rows", z, eps, x_next, guidance, hist, None, mask, z_img, blend_noise, unipc=True)
    L.check(L.load().imd_unipc_step_rows(C.byref(p), _unipc_rows_ptr("unipc_step_rows", coef_rows, p.B), _stream()))
    return z


def unipc_step_rows_at(z, eps, x_next, *, guidance, coef_rows, row_slot, hist=None, mask=None, z_img=None, blend_noise=None):
    """:func:`unipc_step_rows` through a row -> slot map (``imd_unipc_step_rows_at``; the compacting denoising session), with the
    semantics of :func:`sampler_step_rows_at`.  By ROW: ``eps`` [2B,HW,4], ``x_next`` [2B,HW,8], ``coef_rows`` [B,24], a ``guidance``
    tensor [B].  By SLOT: ``z`` [slots,HW,4] (in place), ``hist`` [K,slots,HW,4], ``mask`` / ``z_img`` / ``blend_noise``."""
    slots = z.shape[0]
    rs = _row_slot_ptr("unipc_step_rows_at", row_slot, slots)
    B = row_slot.numel()
    p = _sampler_params("unipc_step_rows_at", z, eps, x_next, guidance, hist, None, mask, z_img, blend_noise, rows=B, unipc=True)
    L.check(L.load().imd_unipc_step_rows_at(C.byref(p), _unipc_rows_ptr("unipc_step_rows_at", coef_rows, B), rs, slots, _stream()))
    return z


# ---- seeded noise that belongs to a request (csrc/noise.hip) ----
NOISE_ROW_WORDS = L.NOISE_ROW_WORDS
NOISE_COUNTER = {"launches": 0}          # imd_noise_rows launches of this process (tests check that the switch-off call makes none)


def noise_key_row(seed, image, draw, active=True):
    """One row of ``imd_noise_rows``: ``[seed_lo, seed_hi, image, draw, active, 0, 0, 0]`` as 8 Python ints below 2^32.  ``seed``: an
    int in [0, 2^64); ``image`` (the index inside num_images_per_prompt) and ``draw`` (0: the initial noise, 1 + i: the variance noise
    of step index i of the request's full schedule): ints in [0, 2^32).  bool, float and anything out of range raise ValueError."""
    for name, v, bits in (("seed", seed, 64), ("image", image, 32), ("draw", draw, 32)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < (1 << bits):
            raise ValueError(f"noise_key_row: {name} must be an int in [0, 2^{bits}), got {v!r}")
    return [seed & 0xFFFFFFFF, seed >> 32, image, draw, 1 if active else 0, 0, 0, 0]


def noise_key_rows(rows, device=None):
    """:func:`noise_key_row` rows as the [rows, 8] int32 tensor ``imd_noise_rows`` reads (the words reinterpreted as int32: torch has
    no arithmetic on uint32); a host tensor when ``device`` is None."""
    import numpy as np
    a = np.asarray(rows, dtype=np.uint32).reshape(-1, NOISE_ROW_WORDS)
    t = torch.from_numpy(a.view(np.int32).copy())
    return t if device is None else t.to(device)


def noise_rows(out, key_rows, *, kind="normal"):
    """Seeded noise of every active row in one launch (``imd_noise_rows``): ``out`` [rows, HW, 4] contiguous on the device -- fp32 for
    ``kind="normal"`` (standard normals by Philox4x32-10 and Box-Muller, |x| <= 5.77), int32 for ``kind="bits"`` (the four raw
    Philox words of each pixel) -- and ``key_rows`` [rows, 8] int32 on the device (:func:`noise_key_rows`).  The value of a pixel
    depends on its key row and its index alone; a row whose ``active`` word is 0 keeps its bytes."""
    if kind not in L.NOISE_KINDS:
        raise L.ImdError(f"noise_rows: unknown kind {kind!r} (one of {sorted(L.NOISE_KINDS)})")
    if not isinstance(out, torch.Tensor) or out.dim() != 3 or out.shape[2] != 4:
        raise L.ImdError(f"noise_rows: out {tuple(getattr(out, 'shape', ()))}: expected [rows, HW, 4]")
    ensure_device(out.device)
    rows, HW = out.shape[0], out.shape[1]
    if (not isinstance(key_rows, torch.Tensor) or key_rows.dtype != torch.int32 or key_rows.numel() != rows * NOISE_ROW_WORDS
            or not key_rows.is_contiguous()):
        raise L.ImdError(f"noise_rows: key_rows must be a contiguous device int32 tensor [{rows}, {NOISE_ROW_WORDS}] "
                         f"(ops.noise_key_rows), got {getattr(key_rows, 'dtype', type(key_rows))} {tuple(getattr(key_rows, 'shape', ()))}")
    p = L.NoiseParams()
    p.out = _dev(out, torch.float32 if kind == "normal" else torch.int32, "out")
    p.key_rows = _dev(key_rows, torch.int32, "key_rows")
    p.rows, p.HW, p.kind = rows, HW, L.NOISE_KINDS[kind]
    L.check(L.load().imd_noise_rows(C.byref(p), _stream()))
    NOISE_COUNTER["launches"] += 1
    return out


# ---- CFG rescale in front of any step (csrc/guidance_rescale.hip) ----
def guidance_rescale(eps, *, guidance, rescale):
    """The CFG rescale of Lin et al. 2023, section 3.4 (diffusers' ``rescale_noise_cfg``) in place on ``eps`` [2B,HW,4] fp32
    (``imd_guidance_rescale``): for every latent row b whose ``rescale`` is not 0, rows b and B + b both receive
    f (eps_u + g (eps_c - eps_u)), f = rescale * std(eps_c) / std(guided) + 1 - rescale -- so the step launch that follows recovers
    that value whatever guidance it is given.  A row with ``rescale`` 0 keeps its bytes.  ``guidance`` / ``rescale``: a float each, or
    a contiguous device fp32 tensor [B] (the conventions of the step wrappers' ``guidance``)."""
    ensure_device(eps.device)
    p = L.GuidanceRescaleParams()
    p.eps = _dev(eps, torch.float32, "eps")
    if eps.dim() != 3 or eps.shape[2] != 4 or eps.shape[0] < 2 or eps.shape[0] % 2:
        raise L.ImdError(f"guidance_rescale: eps {tuple(eps.shape)}: expected [2B, HW, 4]")
    p.B, p.HW = eps.shape[0] // 2, eps.shape[1]
    for name, val in (("guidance", guidance), ("rescale", rescale)):
        if isinstance(val, torch.Tensor):
            if val.dtype != torch.float32 or val.numel() != p.B or not val.is_contiguous():
                raise L.ImdError(f"guidance_rescale: per-row {name} must be a contiguous fp32 tensor of {p.B} values, got "
                                 f"{val.dtype} {tuple(val.shape)}")
            setattr(p, name + "_rows", _dev(val, torch.float32, name))
            setattr(p, name, 0.0)
        else:
            setattr(p, name + "_rows", None)
            setattr(p, name, float(val))
    L.check(L.load().imd_guidance_rescale(C.byref(p), _stream()))
    return eps


# ---------------------------------------------------------------------------------------------
# image input / output (csrc/image.hip; imagdressing_amd/image.py builds the coefficient tables)
# ---------------------------------------------------------------------------------------------
IMAGE_U8, IMAGE_F32_NCHW, IMAGE_16_NHWC8 = 0, 1, 2          # IMD_IMG_*
IMAGE_FORCE_TWO_PASS = 1                                    # IMD_IMG_FORCE_TWO_PASS
IMAGE_TILE_W, IMAGE_TILE_H, IMAGE_LDS_BYTES = 32, 8, 32768  # IMD_IMG_TILE_W / _TILE_H / _LDS_BYTES
IMAGE_IO_COUNTER = {"resample": 0, "resample_single": 0, "resample_two_pass": 0, "pack_u8": 0, "overlay": 0,
                    "inpaint_condition": 0, "mask_filter": 0, "mask_filter_launches": 0}          # calls made (tests, tools/*_bench.py)
IMAGE_MASK_LINE_MAX = 16384                                 # IMD_IMG_MASK_LINE_MAX
IMAGE_MASK_FORCE_GLOBAL = 1                                 # IMD_IMG_MASK_FORCE_GLOBAL


def image_resample(src: torch.Tensor, size: Tuple[int, int], table_h: Optional[dict], table_v: Optional[dict], *, kind: int = IMAGE_U8,
                   a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), crop: Optional[Tuple[int, int, int, int]] = None, binarize: bool = False,
                   dtype=None, out: Optional[torch.Tensor] = None, _force_two_pass: bool = False) -> torch.Tensor:
    """uint8 ``src`` [B, Hin, Win, C] (C = 1 | 3; rows may be strided) -> resized to ``size`` = (Hres, Wres) as Pillow does, then the
    output stage over ``crop`` = (top, left, h, w) of the resized image: IMAGE_U8 uint8 [B, h, w, C], IMAGE_F32_NCHW fp32 [B, C, h, w]
    = v / 255 * a[c] + b[c], IMAGE_16_NHWC8 the same in 16 bits as [B, h, w, 8].  ``table_h`` / ``table_v``: ``image.device_tables`` of
    the axis, None for an axis whose size does not change.  One launch, or two through a uint8 intermediate when the rows a tile needs
    exceed its LDS (``_force_two_pass``: take that road regardless -- tests)."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise L.ImdError(f"src: tensor is on {getattr(src, 'device', type(src))}; imagdressing_amd runs on MI355X only (no CPU path)")
    if src.dtype != torch.uint8 or src.dim() != 4 or src.stride(3) != 1 or src.stride(2) != src.shape[3]:
        raise L.ImdError(f"src: expected uint8 [B, H, W, C] with contiguous rows, got {src.dtype} {tuple(src.shape)} strides {src.stride()}")
    ensure_device(src.device)
    B, Hin, Win, Cc = (int(v) for v in src.shape)
    Hres, Wres = int(size[0]), int(size[1])
    top, left, ch, cw = (0, 0, Hres, Wres) if crop is None else (int(v) for v in crop)
    shape = {IMAGE_U8: (B, ch, cw, Cc), IMAGE_F32_NCHW: (B, Cc, ch, cw), IMAGE_16_NHWC8: (B, ch, cw, 8)}.get(kind)
    if shape is None:
        raise L.ImdError(f"image_resample: unknown output kind {kind}")
    odt = {IMAGE_U8: torch.uint8, IMAGE_F32_NCHW: torch.float32}.get(kind, dtype if out is None else out.dtype)
    if kind == IMAGE_16_NHWC8 and odt not in DTYPE_CODE:
        raise L.ImdError(f"image_resample: an NHWC8 output is bfloat16 or float16 (dtype= or out=), got {odt}")
    if out is None:
        out = torch.empty(shape, dtype=odt, device=src.device)
    elif tuple(out.shape) != shape:
        raise L.ImdError(f"out: expected shape {shape}, got {tuple(out.shape)}")
    p = L.ImageResampleParams()
    p.src, p.src_row_stride, p.src_img_stride = src.data_ptr(), src.stride(1), src.stride(0)
    p.out = _dev(out, odt, "out")
    p.B, p.Hin, p.Win, p.C, p.Hres, p.Wres = B, Hin, Win, Cc, Hres, Wres
    for axis, t, n_in, n_out in (("h", table_h, Win, Wres), ("v", table_v, Hin, Hres)):
        if t is None:
            continue
        if (t["n_in"], t["n_out"]) != (n_in, n_out):
            raise L.ImdError(f"image_resample: the {axis} table maps {t['n_in']} -> {t['n_out']}, the image needs {n_in} -> {n_out}")
        setattr(p, axis + "_xmin", _dev(t["xmin"], torch.int32, axis + "_xmin"))
        setattr(p, axis + "_count", _dev(t["count"], torch.int32, axis + "_count"))
        setattr(p, axis + "_k", _dev(t["k"], torch.int32, axis + "_k"))
        setattr(p, axis + "_kmax", t["kmax"])
        setattr(p, axis + "_taps", t["taps"])
    p.top, p.left, p.crop_h, p.crop_w = top, left, ch, cw
    p.kind, p.binarize, p.flags = kind, int(bool(binarize)), IMAGE_FORCE_TWO_PASS if _force_two_pass else 0
    p.dtype = _code(out, "out") if kind == IMAGE_16_NHWC8 else 0
    for c in range(3):
        p.a[c], p.b[c] = float(a[c]), float(b[c])
    lib = L.load()
    tmp = None
    if table_h is not None and table_v is not None:
        if 0 <= top and ch > 0 and top + ch <= Hres:
            from .image import tile_rows
            p.v_tile_rows = tile_rows(table_v["host"], top, ch, IMAGE_TILE_H)
        if _force_two_pass or p.v_tile_rows * IMAGE_TILE_W * Cc > IMAGE_LDS_BYTES:
            tmp = torch.empty(B, Hin, max(cw, 1), Cc, dtype=torch.uint8, device=src.device)
            p.tmp = tmp.data_ptr()
    form = lib.imd_image_resample_form(C.byref(p))
    L.check(lib.imd_image_resample(C.byref(p), _stream()))
    IMAGE_IO_COUNTER["resample"] += 1
    if table_h is not None and table_v is not None:
        IMAGE_IO_COUNTER["resample_single" if form == 1 else "resample_two_pass"] += 1
    return out


def image_pack_u8(x: torch.Tensor) -> torch.Tensor:
    """16-bit [B, H, W, 4 | 8] (``AutoencoderKL.decode_nhwc``) -> uint8 [B, H, W, 3] = rint(clamp(x / 2 + 0.5, 0, 1) * 255) in fp32"""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[-1] not in (4, 8):
        raise L.ImdError(f"image_pack_u8: expected a 16-bit [B, H, W, 4 | 8] tensor, got {tuple(getattr(x, 'shape', ()))}")
    p = L.ImagePackParams()
    p.src = _dev(x, x.dtype, "x")
    p.dtype = _code(x, "x")
    ensure_device(x.device)
    out = torch.empty(x.shape[0], x.shape[1], x.shape[2], 3, dtype=torch.uint8, device=x.device)
    p.out = out.data_ptr()
    p.B, p.H, p.W, p.ld = (int(v) for v in x.shape)
    L.check(L.load().imd_image_pack_u8(C.byref(p), _stream()))
    IMAGE_IO_COUNTER["pack_u8"] += 1
    return out


def _u8_images(t, name: str, channels: int):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.ImdError(f"{name}: tensor is on {getattr(t, 'device', type(t))}; imagdressing_amd runs on MI355X only (no CPU path)")
    want = 4 if channels else 3
    if t.dtype != torch.uint8 or t.dim() != want or (channels and t.shape[-1] != channels) or not t.is_contiguous():
        raise L.ImdError(f"{name}: expected contiguous uint8 [B, H, W{', %d' % channels if channels else ''}], got {t.dtype} {tuple(t.shape)}")
    return t


def image_overlay(orig: torch.Tensor, mask: torch.Tensor, gen: torch.Tensor, box: Tuple[int, int, int, int],
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Image.composite(orig with gen pasted at the box, orig, mask)`` per byte on the device: uint8 ``orig`` [Bo, H0, W0, 3] and
    ``mask`` [Bo, H0, W0] (Bo = 1: shared by every output, or B), ``gen`` [B, ch, cw, 3] = the generated window at the size of ``box``
    = (x1, y1, x2, y2) -> uint8 [B, H0, W0, 3]: ``orig`` outside the box, ((t >> 8) + t) >> 8 with t = orig (255 - m) + gen m + 128
    inside."""
    orig, gen = _u8_images(orig, "orig", 3), _u8_images(gen, "gen", 3)
    if isinstance(mask, torch.Tensor) and mask.dim() == 4 and mask.shape[-1] == 1:
        mask = mask[..., 0]
    mask = _u8_images(mask, "mask", 0)
    ensure_device(orig.device)
    x1, y1, x2, y2 = (int(v) for v in box)
    B, Bo, H0, W0 = int(gen.shape[0]), int(orig.shape[0]), int(orig.shape[1]), int(orig.shape[2])
    if tuple(mask.shape) != (Bo, H0, W0):
        raise L.ImdError(f"mask: expected {(Bo, H0, W0)} beside orig {tuple(orig.shape)}, got {tuple(mask.shape)}")
    if tuple(gen.shape[1:3]) != (y2 - y1, x2 - x1):
        raise L.ImdError(f"gen: the box {tuple(box)} is {y2 - y1} x {x2 - x1}, gen is {tuple(gen.shape)}")
    if out is None:
        out = torch.empty(B, H0, W0, 3, dtype=torch.uint8, device=orig.device)
    elif tuple(out.shape) != (B, H0, W0, 3):
        raise L.ImdError(f"out: expected shape {(B, H0, W0, 3)}, got {tuple(out.shape)}")
    p = L.ImageOverlayParams()
    p.orig, p.mask, p.gen, p.out = orig.data_ptr(), mask.data_ptr(), gen.data_ptr(), _dev(out, torch.uint8, "out")
    p.B, p.Bo, p.H0, p.W0 = B, Bo, H0, W0
    p.x1, p.y1, p.cw, p.ch = x1, y1, x2 - x1, y2 - y1
    L.check(L.load().imd_image_overlay(C.byref(p), _stream()))
    IMAGE_IO_COUNTER["overlay"] += 1
    return out


def image_inpaint_condition(image: torch.Tensor, mask: torch.Tensor, dtype) -> torch.Tensor:
    """uint8 ``image`` [B, H, W, 3] and ``mask`` [B, H, W] (or [B, H, W, 1]) -> the inpainting ControlNet's condition, ``dtype``
    [B, H, W, 8]: image / 255, -1 in the three channels where mask / 255 > 0.5, channels 3..7 zero."""
    image = _u8_images(image, "image", 3)
    if isinstance(mask, torch.Tensor) and mask.dim() == 4 and mask.shape[-1] == 1:
        mask = mask[..., 0]
    mask = _u8_images(mask, "mask", 0)
    if tuple(mask.shape) != tuple(image.shape[:3]):
        raise L.ImdError(f"mask: expected {tuple(image.shape[:3])} beside image {tuple(image.shape)}, got {tuple(mask.shape)}")
    if dtype not in DTYPE_CODE:
        raise L.ImdError(f"image_inpaint_condition: the output is bfloat16 or float16, got {dtype}")
    ensure_device(image.device)
    out = torch.empty(*image.shape[:3], 8, dtype=dtype, device=image.device)
    p = L.ImageInpaintConditionParams()
    p.image, p.mask, p.out = image.data_ptr(), mask.data_ptr(), out.data_ptr()
    p.B, p.H, p.W = (int(v) for v in image.shape[:3])
    p.dtype = _code(out, "out")
    L.check(L.load().imd_image_inpaint_condition(C.byref(p), _stream()))
    IMAGE_IO_COUNTER["inpaint_condition"] += 1
    return out


def image_mask_filter(src: torch.Tensor, dilate: int = 0, box: Optional[Tuple[int, int, int]] = None, *, out: Optional[torch.Tensor] = None,
                      bounds: bool = False, passes: int = 3, _force_global: bool = False):
    """``ImageFilter.MaxFilter(2 dilate + 1)`` then ``ImageFilter.GaussianBlur`` of uint8 ``src`` [B, H, W] (rows and images may be
    strided, the bytes of a row are contiguous) -> uint8 [B, H, W], Pillow's bytes.  ``box`` = ``image.gaussian_box(radius)`` =
    (r, ww, fw), None: no blur; ``dilate`` = 0: no maximum.  ``out`` may be ``src`` (in place).  ``bounds``: also return int32 [B, 4] =
    (x_min, y_min, x_max, y_max) of the non-zero output pixels, (W, H, -1, -1) for an all-zero image -> (out, bounds)."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise L.ImdError(f"src: tensor is on {getattr(src, 'device', type(src))}; imagdressing_amd runs on MI355X only (no CPU path)")
    if src.dtype != torch.uint8 or src.dim() != 3 or (src.shape[2] > 1 and src.stride(2) != 1):
        raise L.ImdError(f"src: expected uint8 [B, H, W] with contiguous rows, got {src.dtype} {tuple(src.shape)} strides {src.stride()}")
    ensure_device(src.device)
    B, H, W = (int(v) for v in src.shape)
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.uint8, device=src.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != src.device or tuple(out.shape) != (B, H, W)
          or (W > 1 and out.stride(2) != 1)):
        raise L.ImdError(f"out: expected uint8 {(B, H, W)} with contiguous rows on {src.device}, got {getattr(out, 'dtype', None)} "
                         f"{tuple(getattr(out, 'shape', ()))}")
    p = L.ImageMaskFilterParams()
    p.src, p.src_row_stride, p.src_img_stride = src.data_ptr(), src.stride(1), src.stride(0)
    p.out, p.out_row_stride, p.out_img_stride = out.data_ptr(), out.stride(1), out.stride(0)
    p.B, p.H, p.W, p.k, p.passes = B, H, W, int(dilate), int(passes)
    if box is not None:
        p.blur = 1
        p.r, p.ww, p.fw = (int(v) for v in box)
    tmp = None
    if _force_global or H > IMAGE_MASK_LINE_MAX or W > IMAGE_MASK_LINE_MAX:
        tmp = torch.empty(B, H, W, dtype=torch.uint8, device=src.device)
        p.tmp = tmp.data_ptr()
        p.flags = IMAGE_MASK_FORCE_GLOBAL if _force_global else 0
    bnd = torch.empty(B, 4, dtype=torch.int32, device=src.device) if bounds else None
    if bnd is not None:
        p.bounds = bnd.data_ptr()
    lib = L.load()
    form = lib.imd_image_mask_filter_form(C.byref(p))
    L.check(lib.imd_image_mask_filter(C.byref(p), _stream()))
    IMAGE_IO_COUNTER["mask_filter"] += 1
    IMAGE_IO_COUNTER["mask_filter_launches"] += form
    return (out, bnd) if bounds else out


# ---- soft_mask: gray mask levels as per-pixel repaint depth (csrc/soft_mask.hip) ----
SOFT_MASK_COUNTER = {"mask_release": 0, "soft_mask_rows": 0}          # calls made (tests, tools/soft_mask_bench.py)
RELEASE_MAX_STEPS = 65535                                             # a release step is a uint16


def mask_release(src: torch.Tensor, h: int, w: int, n: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 "L" mask window ``src`` [H0, W0] on the device (rows may be strided: a crop window is a view) -> uint16 [h, w], the
    release step of every latent pixel for a run of ``n`` schedule positions (``imd_image_mask_release``): with S the integer sum of
    the pixel's ``adaptive_avg_pool2d`` bin and D = 255 cnt, n - ceil(S n / D) -- ``image.mask_release_reference``, bit for bit."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise L.ImdError(f"src: tensor is on {getattr(src, 'device', type(src))}; imagdressing_amd runs on MI355X only (no CPU path)")
    if src.dtype != torch.uint8 or src.dim() != 2 or (src.shape[1] > 1 and src.stride(1) != 1):
        raise L.ImdError(f"src: expected uint8 [H0, W0] with contiguous rows, got {src.dtype} {tuple(src.shape)} strides {src.stride()}")
    ensure_device(src.device)
    h, w = int(h), int(w)
    if out is None:
        out = torch.empty(max(h, 0), max(w, 0), dtype=torch.uint16, device=src.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint16 or out.device != src.device or out.numel() != h * w
          or not out.is_contiguous()):
        raise L.ImdError(f"out: expected contiguous uint16 of {h * w} values on {src.device}, got {getattr(out, 'dtype', None)} "
                         f"{tuple(getattr(out, 'shape', ()))}")
    p = L.ImageMaskReleaseParams()
    p.src, p.src_row_stride, p.out = src.data_ptr(), src.stride(0), out.data_ptr()
    p.H0, p.W0, p.h, p.w, p.n = int(src.shape[0]), int(src.shape[1]), h, w, int(n)
    L.check(L.load().imd_image_mask_release(C.byref(p), _stream()))
    SOFT_MASK_COUNTER["mask_release"] += 1
    return out


def soft_mask_rows(mask: torch.Tensor, release: torch.Tensor, step_rows: torch.Tensor) -> torch.Tensor:
    """The 0 / 1 blend mask of one step in one launch (``imd_soft_mask_rows``): ``mask`` [B, HW] fp32, ``release`` [B, HW] uint16 and
    ``step_rows`` [B] int32, all contiguous on the device.  Row r with ``step_rows[r]`` >= 0 receives
    ``(step_rows[r] >= release[r]) ? 1 : 0``; a row with a negative entry keeps its bytes (a hard-mask request of the batch)."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2:
        raise L.ImdError(f"soft_mask_rows: mask {tuple(getattr(mask, 'shape', ()))}: expected [B, HW]")
    ensure_device(mask.device)
    B, HW = int(mask.shape[0]), int(mask.shape[1])
    if (not isinstance(release, torch.Tensor) or release.dtype != torch.uint16 or tuple(release.shape) != (B, HW) or not release.is_contiguous()
            or release.device != mask.device):
        raise L.ImdError(f"soft_mask_rows: release must be a contiguous device uint16 tensor [{B}, {HW}], got "
                         f"{getattr(release, 'dtype', type(release))} {tuple(getattr(release, 'shape', ()))}")
    if (not isinstance(step_rows, torch.Tensor) or step_rows.dtype != torch.int32 or step_rows.numel() != B or not step_rows.is_contiguous()):
        raise L.ImdError(f"soft_mask_rows: step_rows must be a contiguous device int32 tensor [{B}], got "
                         f"{getattr(step_rows, 'dtype', type(step_rows))} {tuple(getattr(step_rows, 'shape', ()))}")
    p = L.SoftMaskRowsParams()
    p.mask = _dev(mask, torch.float32, "mask")
    p.release = release.data_ptr()
    p.step_rows = _dev(step_rows, torch.int32, "step_rows")
    p.B, p.HW = B, HW
    L.check(L.load().imd_soft_mask_rows(C.byref(p), _stream()))
    SOFT_MASK_COUNTER["soft_mask_rows"] += 1
    return mask


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    ensure_device(t.device)
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    L.check(L.load().imd_timestep_embedding(_dev(t, torch.float32, "t"), out.data_ptr(), t.shape[0], dim, _stream()))
    return out


def add(a: torch.Tensor, b: torch.Tensor, b_scale: float = 1.0, out=None) -> torch.Tensor:
    ensure_device(a.device)
    Cc = a.shape[-1]
    rows = a.numel() // Cc
    if out is None:
        out = torch.empty_like(a)
    dt = a.dtype
    L.check(L.load().imd_add(_dev(a, dt, "a"), Cc, _dev(b, dt, "b"), Cc, _dev(out, dt, "out"), Cc, rows, Cc,
                             b_scale, _code(a, "a"), _stream()))
    return out


def concat_channels(a: torch.Tensor, b: torch.Tensor, b_add: Optional[torch.Tensor] = None, gn_stats_groups: int = 0) -> torch.Tensor:
    """cat([a, b (+ b_add)], channel) for NHWC tensors [..., Ca] and [..., Cb].

    ``gn_stats_groups`` = G (4-D operands [B, H, W, C]): the launch also writes the GroupNorm(G) statistics of its output, which ride on the
    returned tensor (``_imd_gn_stats``) exactly as a convolution's do -- the :func:`group_norm` behind an up block's concatenation then
    normalises only.  Same partials as the statistics launch would write (same chunking and order): bit-identical either way."""
    ensure_device(a.device)
    Ca, Cb = a.shape[-1], b.shape[-1]
    rows = a.numel() // Ca
    dt = a.dtype
    out = torch.empty(a.shape[:-1] + (Ca + Cb,), dtype=dt, device=a.device)
    lib = L.load()
    b_rows = b.numel() // Cb            # b may hold HALF the rows: one skip tensor for both (identical) halves of a CFG batch
    if b_rows * Cb != b.numel() or b_rows == 0 or rows % b_rows or (b_add is not None and b_add.numel() != rows * Cb):
        raise L.ImdError(f"concat_channels: operands disagree on the row count ({rows} rows of {Ca} + {Cb} channels, b has {b_rows})")
    G = gn_stats_groups
    if G and FUSED_CONCAT_STATS and FUSED_GN_STATS and a.dim() == 4 and b.dim() == 4 and (Ca + Cb) % G == 0:
        B = a.shape[0]
        HW = rows // B
        cpg = (Ca + Cb) // G
        nparts = lib.imd_groupnorm_parts(B, HW, Ca + Cb)
        if nparts > 0 and b_rows % HW == 0 and G <= 64 and (cpg >= 8 or cpg == 4):
            part = torch.empty((B, nparts, G, 2), dtype=torch.float32, device=a.device)
            L.check(lib.imd_concat2_gn_stats(_dev(a, dt, "a"), Ca, _dev(b, dt, "b"), Cb, _opt(b_add, dt, "b_add"), out.data_ptr(), B, HW, b_rows // HW, G,
                                             part.data_ptr(), _code(a, "a"), _stream()))
            out._imd_gn_stats = (part, nparts, G)
            return out
    L.check(lib.imd_concat2(_dev(a, dt, "a"), Ca, _dev(b, dt, "b"), Cb, _opt(b_add, dt, "b_add"), out.data_ptr(), rows, b_rows, _code(a, "a"), _stream()))
    return out


FREEU_COUNTER = {"launches": 0}          # imd_concat2_freeu launches of this process (tests count the full / shallow forwards of DeepCache with it)


def concat_channels_freeu(a: torch.Tensor, b: torch.Tensor, b_add: Optional[torch.Tensor], H: int, W: int, backbone_scale: float,
                          skip_scale: float, gn_stats_groups: int = 0) -> torch.Tensor:
    """:func:`concat_channels` with FreeU (diffusers 0.24 ``apply_freeu``) applied to its operands, in the same single launch
    (``imd_concat2_freeu``): ``a`` [B, H, W, Ca] has its lower channel half multiplied by ``backbone_scale``; the skip ``b (+ b_add)``
    [B, H, W, Cb] goes through ``fourier_filter(threshold=1, scale=skip_scale)`` per (image, channel) map, computed in fp32 in its closed
    form (seven sums per map, no FFT).  ``gn_stats_groups`` = G: the GroupNorm(G) statistics of the stored tensor ride on the result
    (``_imd_gn_stats``) under the conditions of :func:`concat_channels`; elsewhere the launch writes none and :func:`group_norm` runs its
    own pass.  Both scales 1.0 store :func:`concat_channels`' bits."""
    ensure_device(a.device)
    dt = a.dtype
    H, W = int(H), int(W)
    if a.dim() != 4 or b.dim() != 4 or tuple(a.shape[:3]) != tuple(b.shape[:3]) or tuple(a.shape[1:3]) != (H, W):
        raise L.ImdError(f"concat_channels_freeu: operands must be [B, {H}, {W}, C] with one B (the skip holds every image), got {tuple(a.shape)} and {tuple(b.shape)}")
    if b_add is not None and tuple(b_add.shape) != tuple(b.shape):
        raise L.ImdError(f"concat_channels_freeu: b_add {tuple(b_add.shape)} must have the skip's shape {tuple(b.shape)}")
    B, Ca, Cb = int(a.shape[0]), int(a.shape[-1]), int(b.shape[-1])
    out = torch.empty((B, H, W, Ca + Cb), dtype=dt, device=a.device)
    lib = L.load()
    G = int(gn_stats_groups)
    part, nparts = None, 0
    if G and FUSED_CONCAT_STATS and FUSED_GN_STATS and (Ca + Cb) % G == 0:
        nparts = lib.imd_concat2_freeu_parts(B, H, W, Ca, Cb, G)
        if nparts > 0:
            part = torch.empty((B, nparts, G, 2), dtype=torch.float32, device=a.device)
    L.check(lib.imd_concat2_freeu(_dev(a, dt, "a"), Ca, _dev(b, dt, "b"), Cb, _opt(b_add, dt, "b_add"), out.data_ptr(), B, H, W, B, G if part is not None else 0,
                                  None if part is None else part.data_ptr(), float(backbone_scale), float(skip_scale), _code(a, "a"), _stream()))
    FREEU_COUNTER["launches"] += 1
    if part is not None:
        out._imd_gn_stats = (part, nparts, G)
    return out


def repeat_batch(x: torch.Tensor, times: int = 2) -> torch.Tensor:
    """cat([x] * times, dim=0) for a contiguous NHWC tensor (strided 2-D copies)."""
    ensure_device(x.device)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    out = torch.empty((x.shape[0] * times,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    src = _dev(x, x.dtype, "x")
    for i in range(times):
        L.check(L.load().imd_copy2d(src, Cc, out.data_ptr() + 2 * i * rows * Cc, Cc, rows, Cc, _stream()))
    return out


def copy_into(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst <- src for two contiguous 16-bit tensors of one shape (one strided 2-D copy, as :func:`repeat_batch`): a snapshot of an
    activation into storage the caller owns."""
    ensure_device(src.device)
    if dst.shape != src.shape or dst.dtype != src.dtype or src.dtype not in DTYPE_CODE or not dst.is_contiguous():
        raise L.ImdError(f"copy_into: {tuple(src.shape)} {src.dtype} -> {tuple(dst.shape)} {dst.dtype}: shapes and 16-bit element types must agree")
    Cc = src.shape[-1]
    L.check(L.load().imd_copy2d(_dev(src, src.dtype, "src"), Cc, dst.data_ptr(), Cc, src.numel() // Cc, Cc, _stream()))
    return dst


def f32_to_16(a: torch.Tensor, dtype=bf16) -> torch.Tensor:
    ensure_device(a.device)
    out = torch.empty(a.shape, dtype=dtype, device=a.device)
    L.check(L.load().imd_f32_to_16(_dev(a, torch.float32, "a"), out.data_ptr(), a.numel(), DTYPE_CODE[dtype], _stream()))
    return out


def concat_tokens(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """cat([a, b], dim=1) for [B, La, C] and [B, Lb, C] (one strided 2-D copy per operand)."""
    ensure_device(a.device)
    B, La, Cc = a.shape
    Lb = b.shape[1]
    dt = a.dtype
    _code(a, "a")
    out = torch.empty(B, La + Lb, Cc, dtype=dt, device=a.device)
    lib = L.load()
    ld = (La + Lb) * Cc
    L.check(lib.imd_copy2d(_dev(a, dt, "a"), La * Cc, out.data_ptr(), ld, B, La * Cc, _stream()))
    L.check(lib.imd_copy2d(_dev(b, dt, "b"), Lb * Cc, out.data_ptr() + 2 * La * Cc, ld, B, Lb * Cc, _stream()))
    return out
