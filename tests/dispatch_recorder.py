"""What ``ops.conv_gemm`` DECIDES, observed without a GPU.  ``record(ops, lib)`` runs a list of problems through the dispatcher with
``ops.L.load`` swapped for a proxy: the library's pure queries (``*_supported``, ``*_parts``, ``auto_cfg``, ``auto_split``) are forwarded, every
other symbol is a stub that notes the call and returns 0 -- no launching entry point of the real library is ever reached (the operands are
uninitialised CPU tensors: a launch would fault).  ``tests/golden/dispatch_decisions.json`` holds the record of the commit BEFORE the tile-config
tables were introduced; tests/test_host_logic.py re-records and requires equality, entry for entry.  Regenerate (from the repository root):

    python -m tests.dispatch_recorder tests/golden/dispatch_decisions.json

One launch is recorded as ``[entry, cfg, split_k, gn_stats_groups, res_rows, gn_in fused, gn_out fused, workspace given, counters given]`` for
``imd_conv_gemm`` (entry 0) and ``imd_row_linear`` (entry 1, cfg = -2); the GroupNorm / copy launches the dispatcher puts in front where it cannot fuse
are ``[2]`` (``imd_groupnorm``) and ``[3]`` (``imd_copy2d``)."""
import ctypes as C
import hashlib
import json
import sys
from types import SimpleNamespace

import torch

from tests import dispatch_cases as DC
from tests import geometry_cases as GC

ENTRY = {"imd_conv_gemm": 0, "imd_row_linear": 1, "imd_groupnorm": 2, "imd_copy2d": 3}
# the queries a tile choice may ask (a decision-cache hit asks none of them); the two fusion queries (imd_row_linear_gn_in_supported,
# imd_conv_gemm_gn_out_supported) depend on what rides on the operands of one call and are asked per call
CHOICE_QUERIES = ("imd_conv_patch_supported", "imd_conv_patch2_supported", "imd_conv_patch3_supported", "imd_conv_patch4_supported",
                  "imd_conv_img_supported", "imd_row_linear_supported", "imd_gemm_dma_supported")
PURE = CHOICE_QUERIES + ("imd_conv_gemm_auto_cfg", "imd_conv_gemm_auto_split", "imd_conv_gemm_stats_parts", "imd_conv_patch_stats_parts",
                         "imd_conv_gemm_gn_out_supported", "imd_row_linear_gn_in_supported", "imd_groupnorm_workspace_floats", "imd_groupnorm_parts",
                         "imd_attn_padded_dims", "imd_abi_version", "imd_last_error", "imd_get_tuning")
SWITCHES = ("FUSED_GN_FINISH", "GENERIC_GN_STATS", "SPLITK_IN_KERNEL", "PATCH_CONV")      # the first three recorded switched ON, PATCH_CONV switched OFF
DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))
FAKE = 0x10000          # every "device pointer" the dispatcher sees: never dereferenced
GN = 32                 # GroupNorm groups of the product
HEADS = 8


class Proxy:
    """The loaded library with every non-pure symbol replaced by a recording stub."""

    def __init__(self, lib):
        self._lib, self.launches, self.queries, self.blocks = lib, [], 0, []

    def __getattr__(self, name):
        if name in PURE:
            fn = getattr(self._lib, name)
            if name not in CHOICE_QUERIES:
                return fn

            def asked(*a):
                self.queries += 1
                return fn(*a)
            return asked
        if name not in ENTRY:
            raise AssertionError(f"the dispatcher reached {name}: neither a pure query nor a launch this recorder knows")

        def stub(*a):
            if ENTRY[name] < 2:
                p = a[0]._obj
                cfg = a[1] if name == "imd_conv_gemm" else -2
                self.launches.append([ENTRY[name], cfg, p.split_k, p.gn_stats_groups, p.res_rows, int(bool(p.gn_in_partial)), int(bool(p.gn_out_gamma)),
                                      int(bool(p.splitk_ws)), int(bool(p.splitk_counters))])
                q = type(p)()
                C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
                self.blocks.append(q)
            else:
                self.launches.append([ENTRY[name]])
            return 0
        return stub


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the problem list: (id, spec); a spec is what _call() turns into one ops.conv_gemm call
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _spec(M, N, Cin, taps=1, stride=1, ups=0, B=1, Hin=1, Win=1, Hout=1, Wout=1, **kw):
    return dict(M=M, N=N, Cin=Cin, taps=taps, stride=stride, ups=ups, B=B, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, **kw)


def _heads_spec(M, Cc, B):
    D, HW = Cc // HEADS, M // B
    return _spec(M, 3 * Cc, Cc, B=B, Hin=HW, Hout=HW, heads=(Cc, HEADS, D))


def table_problems(table):
    """Every case of tests/dispatch_cases.py, as the sweep launches it; behind every case whose tabulated config is a row-resident projection
    (12 / 13 / 14) the same problem with ``gn_in`` (statistics riding on ``x``) and with a half-height periodic residual."""
    out = []
    for c in DC.cases(table):
        geo = dict(M=c.M, N=c.N, Cin=c.Cin, taps=c.taps, stride=c.stride, ups=c.ups, B=c.B, Hin=c.Hin, Win=c.Win, Hout=c.Hout, Wout=c.Wout)
        if c.form == "geglu":
            out.append((c.id, dict(geo, bias=True, act=2)))
        elif c.form == "heads":
            out.append((c.id, dict(geo, bias=True, heads=(c.K, HEADS, c.K // HEADS))))
        else:
            out.append((c.id, dict(geo, bias=True, res=c.M, rowvec=c.rowvec, gn_stats=c.gn_groups)))
            if c.table_cfg in (12, 13, 14):
                # Transformer2DModel.proj_in on a map: two images of M / 2 pixels (one where M is odd)
                B = 1 if c.M % 2 else 2
                out.append((c.id + "+gn_in", dict(geo, B=B, Hout=c.M // B, Hin=c.M // B, bias=True, gn_in=True, x_stats=4)))
                if c.M % 2 == 0:
                    out.append((c.id + "+periodic", dict(geo, bias=True, res=c.M // 2)))
    return out


def off_table_problems():
    """The layers of one UNet level at every level of tests/geometry_cases.py (the CFG batch: 2 x images)."""
    out = []
    for case in GC.GEOMETRY_CASES:
        for lv in GC.levels(case):
            Cc, H, W, B = lv.channels, lv.H, lv.W, 2 * case.images
            M, HW = lv.cfg_rows, lv.tokens
            pre = f"{case.id}/L{lv.level}"
            conv = dict(taps=9, B=B, Hin=H, Win=W, Hout=H, Wout=W, bias=True)
            lin = dict(B=B, Hin=HW, Hout=HW, bias=True)
            out.append((f"{pre}/conv3x3", _spec(M, Cc, Cc, rowvec=True, res=M, gn_stats=GN, **conv)))
            out.append((f"{pre}/conv1", _spec(M, Cc, Cc, rowvec=True, gn_out=True, gn_stats=GN, **conv)))
            out.append((f"{pre}/conv3x3 2C", _spec(M, Cc, 2 * Cc, rowvec=True, gn_stats=GN, **conv)))
            if H % 2 == 0 and W % 2 == 0:
                out.append((f"{pre}/down", _spec(M // 4, Cc, Cc, taps=9, stride=2, B=B, Hin=H, Win=W, Hout=H // 2, Wout=W // 2, bias=True, gn_stats=GN)))
            out.append((f"{pre}/up", _spec(4 * M, Cc, Cc, taps=9, ups=1, B=B, Hin=H, Win=W, Hout=2 * H, Wout=2 * W, bias=True)))
            out.append((f"{pre}/proj_out", _spec(M, Cc, Cc, res=M, **lin)))
            out.append((f"{pre}/proj_out periodic", _spec(M, Cc, Cc, res=M // 2, **lin)))
            out.append((f"{pre}/proj_in gn_in", _spec(M, Cc, Cc, B=B, Hin=H, Win=W, Hout=H, Wout=W, bias=True, gn_in=True, x_stats=4)))
            out.append((f"{pre}/proj_in gn_in no stats", _spec(M, Cc, Cc, B=B, Hin=H, Win=W, Hout=H, Wout=W, bias=True, gn_in=True)))
            out.append((f"{pre}/geglu", _spec(M, 8 * Cc, Cc, act=2, **lin)))
            out.append((f"{pre}/ff_out", _spec(M, Cc, 4 * Cc, res=M, **lin)))
            out.append((f"{pre}/qkv", _heads_spec(M, Cc, B)))
            if Cc == 320:
                out.append((f"{pre}/ln to_q", _spec(M, Cc, Cc, ln_eps=1e-5, heads=(Cc, HEADS, Cc // HEADS), n_dests=1, **lin)))
                out.append((f"{pre}/ln proj periodic", _spec(M, Cc, Cc, ln_eps=1e-5, res=M // 2, **lin)))
        # the layers around the levels: conv_in / conv_out of the latent, the time-embedding projection with its fp32 output
        H, W, B = case.h, case.w, 2 * case.images
        out.append((f"{case.id}/conv_in", _spec(B * H * W, 320, 8, taps=9, B=B, Hin=H, Win=W, Hout=H, Wout=W, bias=True, gn_stats=GN)))
        out.append((f"{case.id}/conv_out", _spec(B * H * W, 4, 320, taps=9, B=B, Hin=H, Win=W, Hout=H, Wout=W, bias=True, out_f32=True)))
        out.append((f"{case.id}/temb", _spec(B, 1280, 1280, bias=True, act=1, out_f32=True)))
    return out


def problems(table):
    return table_problems(table) + off_table_problems()


def switch_matters(switch, s):
    """Can module switch ``switch`` change what the dispatcher does with spec ``s``?"""
    if s.get("ln_eps") is not None:
        return False
    if switch == "FUSED_GN_FINISH":
        return bool(s.get("gn_out"))
    if switch == "GENERIC_GN_STATS":
        return bool(s.get("gn_stats"))
    if switch == "SPLITK_IN_KERNEL":
        return s.get("heads") is None and s.get("act", 0) != 2
    return s["taps"] == 9 and s["stride"] == 1          # PATCH_CONV


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _empty(*shape, dt=torch.float32):
    return torch.empty(shape, dtype=dt)


def operands(s, dt):
    """(x, w, keyword arguments) of the ``ops.conv_gemm`` call of spec ``s``: uninitialised CPU tensors of the right sizes."""
    M, N, Cin, taps, B = s["M"], s["N"], s["Cin"], s["taps"], s["B"]
    K = taps * Cin
    x = _empty(B * s["Hin"] * s["Win"] if taps == 9 else M, Cin, dt=dt)
    if s.get("x_stats"):
        x._imd_gn_stats = (_empty(B, s["x_stats"], GN, 2), s["x_stats"], GN)
    kw = dict(M=M, N=N, Cin=Cin, taps=taps, Hin=s["Hin"], Win=s["Win"], Hout=s["Hout"], Wout=s["Wout"], stride=s["stride"], ups=bool(s["ups"]),
              act=s.get("act", 0), out_f32=bool(s.get("out_f32")), ln_eps=s.get("ln_eps"), gn_stats_groups=s.get("gn_stats", 0))
    if s.get("bias"):
        kw.update(bias=_empty(N))
    if s.get("rowvec"):
        kw.update(rowvec=_empty(B, N), rowvec_stride=N)
    if s.get("res"):
        kw.update(res=_empty(s["res"], N, dt=dt))
    if s.get("gn_in"):
        kw.update(gn_in=(_empty(Cin), _empty(Cin), 1e-6, False, GN))
    if s.get("gn_out"):
        kw.update(gn_out=(_empty(N), _empty(N), 1e-5, True, GN))
    if s.get("heads"):
        Cc, H, D = s["heads"]
        HW = M // B
        dests = [(_empty(B, H, HW, D, dt=dt), 0, D, HW, 0.125), (_empty(B, H, HW, D, dt=dt), 0, D, HW, 1.0), (_empty(B, H, D, HW, dt=dt), 1, D, HW, 1.0)]
        kw.update(heads=dict(C=Cc, H=H, D=D, dests=dests[:s.get("n_dests", 3)]))
    return x, _empty(N, K, dt=dt), kw


def _call(ops, s, dt):
    x, w, kw = operands(s, dt)
    return ops.conv_gemm(x, w, **kw)


class harness:
    """``with harness(ops, lib) as h``: the dispatcher runs on CPU tensors against ``h.proxy``; ``h.lookups`` counts tuning-table lookups."""

    def __init__(self, ops, lib):
        self.ops, self.proxy, self.lookups = ops, Proxy(lib), 0

    def __enter__(self):
        ops = self.ops
        self.saved = {n: getattr(ops, n) for n in ("ensure_device", "_dev", "_stream", "splitk_workspace", "splitk_counters", "_gemm_table", "GEMM_TRACE", "GEMM_EVENT_HOOK") + SWITCHES}
        self.load, self.ws = ops.L.load, set(ops._ws)
        table, scratch = ops._gemm_table, SimpleNamespace(data_ptr=lambda: FAKE)

        def counted_table():
            self.lookups += 1
            return table()
        ops.ensure_device = lambda device: None
        ops._dev = lambda t, dtype, name: FAKE
        ops._stream = lambda: 0
        ops.splitk_workspace = ops.splitk_counters = lambda *a: scratch
        ops._gemm_table = counted_table
        ops.GEMM_TRACE = ops.GEMM_EVENT_HOOK = None
        ops.L.load = lambda: self.proxy
        table()                 # (loaded before the first problem: the identity of the table is part of the decision cache's key)
        return self

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            setattr(self.ops, n, v)
        self.ops.L.load = self.load
        self.ops._CFG_DECISIONS.clear()
        for k in set(self.ops._ws) - self.ws:        # (the GroupNorm partials of the unfused gn_in road: CPU tensors)
            del self.ops._ws[k]
        return False

    def decide(self, spec, dt):
        """One problem, decision cache cleared, then once more with the cache kept: (launches, launches of the second call, choice queries and
        table lookups of the second call)."""
        self.ops._CFG_DECISIONS.clear()
        self.proxy.launches = []
        _call(self.ops, spec, dt)
        first, self.proxy.launches = self.proxy.launches, []
        q0, l0 = self.proxy.queries, self.lookups
        _call(self.ops, spec, dt)
        return first, self.proxy.launches, (self.proxy.queries - q0, self.lookups - l0)


def _digest(names):
    return hashlib.sha1("\n".join(names).encode()).hexdigest()[:16]


# parameter blocks of the pure-answer table: the block the dispatcher handed the library for these problems (bf16, default switches)
BLOCK_PROBLEMS = ("16x16/L0/conv3x3", "16x16/L2/conv3x3", "8x8/L3/conv1", "24x40 x3/L0/conv3x3 2C", "32x32 x5/L1/down", "16x32/L0/proj_out", "32x32 x5/L0/proj_in gn_in",
                  "24x40 x3/L1/proj_in gn_in", "32x32 x5/L2/proj_in gn_in", "16x32/L1/geglu", "32x8/L0/qkv", "16x16/conv_in", "8x8/conv_out", "16x16/temb", "32x32 x5/L3/ff_out")


def pure_answers(lib, blocks, mn):
    """The library's pure answers per tile config -1..33 over ``blocks`` (each also asked K-sliced, with and without the in-kernel sum, where the epilogue allows K slices), and its
    heuristic tile for every (M, N) of ``mn``."""
    rows = []
    for p0 in blocks:
        for split, counters in ((1, None), (4, None), (4, FAKE)):        # un-split, K-sliced, K-sliced with the in-kernel sum asked for
            if split > 1 and (p0.mode == 1 or p0.act == 2):
                continue
            row = []
            for cfg in range(-1, 34):
                p = type(p0)()
                C.memmove(C.byref(p), C.byref(p0), C.sizeof(p0))
                p.split_k, p.splitk_ws, p.splitk_counters, p.gn_stats_out, p.gn_stats_groups = split, FAKE, counters, None, GN
                parts = lib.imd_conv_gemm_stats_parts(C.byref(p), cfg)
                p.gn_stats_groups = 0
                p.gn_in_partial, p.gn_in_gamma, p.gn_in_beta, p.gn_in_nparts, p.gn_in_groups = FAKE, FAKE, FAKE, 4, GN
                gn_in = lib.imd_row_linear_gn_in_supported(C.byref(p), cfg)
                p.gn_in_partial, p.gn_in_nparts, p.gn_in_groups = None, 0, 0
                p.gn_out_gamma, p.gn_out_beta, p.gn_out_groups = FAKE, FAKE, GN
                row.append([parts, lib.imd_conv_gemm_auto_split(p.M, p.N, p.K, cfg), int(gn_in), int(lib.imd_conv_gemm_gn_out_supported(C.byref(p)))])
            rows.append(row)
    return dict(per_cfg=rows, auto_cfg=[lib.imd_conv_gemm_auto_cfg(M, N) for M, N in mn])


def record(ops, lib, table=None):
    """-> (the JSON-ready record, [(section, problem id, launches of the second call where they differ else None, (choice queries, table lookups)
    of the second call) ...] for every problem whose second call, decision cache kept, launched something else or asked anything)."""
    table = DC.load_table() if table is None else table
    probs = problems(table)
    rec = dict(problems=len(probs), ids=_digest([i for i, _ in probs]), sections={})
    bad = []
    with harness(ops, lib) as h:
        blocks = {}
        for switch in (None,) + SWITCHES:
            if switch is not None:
                setattr(ops, switch, switch != "PATCH_CONV")
            picked = [(i, s) for i, s in probs if switch is None or switch_matters(switch, s)]
            for dname, dt in DTYPES:
                got = []
                for pid, spec in picked:
                    h.proxy.blocks = []
                    first, second, asked = h.decide(spec, dt)
                    got.append(first)
                    if second != first or asked != (0, 0):
                        bad.append((f"{switch or 'default'}/{dname}", pid, None if second == first else second, asked))
                    if switch is None and dname == "bf16" and pid in BLOCK_PROBLEMS:
                        blocks[pid] = h.proxy.blocks[-1]
                rec["sections"][f"{switch or 'default'}/{dname}"] = dict(ids=_digest([i for i, _ in picked]), launches=got)
            if switch is not None:
                setattr(ops, switch, h.saved[switch])
        missing = [i for i in BLOCK_PROBLEMS if i not in blocks]
        assert not missing, f"BLOCK_PROBLEMS names problems the list does not hold: {missing}"
    mn = sorted({(s["M"], s["N"]) for _, s in probs})
    rec["pure"] = pure_answers(lib, [blocks[i] for i in BLOCK_PROBLEMS], mn)
    return rec, bad


def section_ids(table, section):
    """Problem ids of a section of the record, in its order (for a readable failure message)."""
    switch = section.split("/")[0]
    return [i for i, s in problems(table) if switch == "default" or switch_matters(switch, s)]


if __name__ == "__main__":
    from imagdressing_amd import _lib, ops as _ops
    rec, bad = record(_ops, _lib.load())
    differs = [b for b in bad if b[2] is not None]
    assert not differs, differs[:5]
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v["launches"]) for k, v in rec["sections"].items()})
