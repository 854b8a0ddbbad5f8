"""Every entry of the GEMM / conv tuning table, launched the way the product launches it (``ops.conv_gemm(cfg=-1, split_k=0)``: the
dispatcher reads ``gemm_tuning.json``) and compared over the WHOLE output with an fp32 computation written here from plain torch.

Per case (tests/dispatch_cases.py turns the table into cases): which kernel ran (one launch; its (tile config, K slices) against the
table's choice), values at the bar of tests/test_kernels_gpu.py, GroupNorm statistics where the launch hands them on, a sentinel tail
behind the output, and a second identical call.  The shapes the table does NOT hold are collected from one denoising step of each
benchmarked workload (``ops.GEMM_TRACE``) and replayed the same way.  The full-width workloads OFF the benchmarked geometries
(tests/geometry_cases.py) are traced too: there EVERY distinct problem is replayed, table hits included -- a hit from another map is the
dispatcher's ``*_supported`` back-out path -- and two of them once more with the decision cache kept across problems.  The last test prints
the module's summary (``-rA``)."""
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.dispatch_cases import HEADS, cases, load_table, lookup_key
from tests.geometry_cases import GEOMETRY_CASES, workload_kwargs
from tests.test_kernels_gpu import TOL, assert_close

pytestmark = pytest.mark.gpu

bf16, f16 = torch.bfloat16, torch.float16
TABLE = load_table()
CASES = cases(TABLE)
# row_qkv.hip (tile config 15) has only the head-split epilogue: the plain form of these two entries goes to the library heuristic
EXPECTED_FALLBACKS = {"32768,960,320,1,1,0", "55296,960,320,1,1,0"}
SENTINEL = -1234.0
DEV = "cuda"
Q_SCALE = 0.3

RECORDS = {}            # (dtype name, case id) -> dict(launched=(cfg, split), tabulated=bool, stats=str)
MISSES = {}             # workload -> list of untabulated problem descriptions
REFUSED = []            # launches of a tile config whose *_supported query refuses the problem: (key, cfg, split, query)
CACHE_KEPT = {}         # workload -> problems replayed with the decision cache kept
T0 = []


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    T0.append(time.time())
    return o


# ------------------------------------------------------------------------------------------
# the reference: plain torch, fp32 (or whatever the operands are), nothing from imagdressing_amd
# ------------------------------------------------------------------------------------------
def ref_gemm(x, w, *, taps, stride, ups, B, Hin, Win, Hout, Wout, Cin, pad_br_only=False):
    """[M, N] = A @ w^T where A is ``x`` [M, K] (taps == 1) or the implicit im2col of the NHWC map ``x`` [B, Hin, Win, Cin] (taps == 9:
    3x3, zero padding 1, optional nearest 2x upsample first), summed tap by tap; ``w`` is [N, taps * Cin] with the tap outermost in K."""
    if taps == 1:
        return x.reshape(-1, Cin) @ w.t()
    x = x.reshape(B, Hin, Win, Cin)
    if ups:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    xp = F.pad(x, (0, 0, 0, 1, 0, 1) if pad_br_only else (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(B * Hout * Wout, w.shape[0], dtype=x.dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, ky: ky + stride * (Hout - 1) + 1: stride, kx: kx + stride * (Wout - 1) + 1: stride, :]
            t = ky * 3 + kx
            acc.addmm_(sl.reshape(-1, Cin), w[:, t * Cin: (t + 1) * Cin].t())
    return acc


def ref_geglu(base):
    return base[:, 0::2] * F.gelu(base[:, 1::2])


def _gen(case_id, dt):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(f"{case_id}/{dt}".encode()))


def _randn(g, *shape, scale=1.0, dt=torch.float32):
    t = torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32)
    return (t * scale if scale != 1.0 else t).to(dt)


# the library's own answer to "does this tile config take this problem" (the queries ops.conv_gemm re-checks a table entry with)
SUPPORT_QUERY = {5: "imd_conv_patch_supported", 21: "imd_conv_patch2_supported", 22: "imd_conv_patch3_supported", 23: "imd_conv_patch4_supported",
                 24: "imd_conv_img_supported", **{c: "imd_row_linear_supported" for c in (12, 13, 14, 15)},
                 **{c: "imd_gemm_dma_supported" for c in (16, 17, 19, 25, 27, 30, 31, 32)}}


class _QueryingLib:
    """The loaded library with ``imd_conv_gemm`` preceded by the ``*_supported`` query of the tile config about to run, on the very parameter block."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def imd_conv_gemm(self, pref, cfg, stream):
        q = SUPPORT_QUERY.get(cfg)
        p = pref._obj
        split = p.split_k
        if q == "imd_gemm_dma_supported" and cfg != 16:     # only the 256 x 256 tile (16) excludes K slices: the library asks on behalf of the other tiles with split_k = 1 (gemm_dma.hip)
            p.split_k = 1
        ok = q is None or bool(getattr(self._lib, q)(pref))
        p.split_k = split
        if not ok:
            self._log.append((f"{p.M},{p.N},{p.K},{p.taps},{p.stride},{p.ups}|{p.Hout}x{p.Wout}", cfg, p.split_k, q))
        return self._lib.imd_conv_gemm(pref, cfg, stream)


def _launch(ops_mod, kwargs_fn, keep_cache=False):
    """One dispatcher call under the event hook, decision cache cleared (or kept): (result, [(key, cfg, split), ...] launches).  A launch the
    library's own ``*_supported`` query refuses lands in ``REFUSED``."""
    hook = ops_mod.GEMM_EVENT_HOOK
    if not keep_cache:
        ops_mod._CFG_DECISIONS.clear()
    ops_mod.GEMM_EVENT_HOOK = {}
    load = ops_mod.L.load
    proxy = _QueryingLib(load(), REFUSED)
    ops_mod.L.load = lambda: proxy
    try:
        r = kwargs_fn()
        seen = [k for k, ev in ops_mod.GEMM_EVENT_HOOK.items() for _ in ev]
    finally:
        ops_mod.GEMM_EVENT_HOOK = hook
        ops_mod.L.load = load
    return r, seen


def _check_stats(out, B, HW, N, split, what):
    st = getattr(out, "_imd_gn_stats", None)
    if st is None:
        return "none"
    part, nparts, G = st
    assert tuple(part.shape) == (B, nparts, G, 2), f"{what}: statistics shaped {tuple(part.shape)}"
    folded = part.double().sum(1)
    o = out.double().view(B, HW, G, N // G)
    n = HW * (N // G)
    mean, sq = o.mean((1, 3)), (o * o).mean((1, 3))
    if split > 1:       # the finish launch of the K slices: bars of test_splitk_finish_groupnorm_statistics
        assert torch.allclose(folded[..., 0] / n, mean, atol=1e-4), f"{what}: group means (finish launch)"
        assert torch.allclose(folded[..., 1] / n, sq, rtol=1e-4, atol=1e-4), f"{what}: group second moments (finish launch)"
        return "finish"
    # an un-split epilogue: bars of test_conv3x3_epilogue_groupnorm_statistics
    assert torch.allclose(folded[..., 0] / n, mean, atol=2e-3), f"{what}: group means (epilogue)"
    assert torch.allclose(folded[..., 1] / n, sq, rtol=5e-3, atol=2e-3), f"{what}: group second moments (epilogue)"
    return "epilogue"


def _act(ops, act, t):
    if act == ops.ACT_SILU:
        return F.silu(t)
    if act == ops.ACT_GELU:
        return F.gelu(t)
    if act == ops.ACT_QUICK_GELU:
        return t * torch.sigmoid(1.702 * t)
    if act == ops.ACT_GEGLU:
        return ref_geglu(t)
    assert act == ops.ACT_NONE, f"activation code {act}"
    return t


def run_problem(ops, dt, tag, *, M, N, Cin, taps, stride, ups, B, Hin, Win, Hout, Wout, bias=True, res=True, res_rows=0, rowvec=False,
                rowvec_shared=False, act=0, gn_groups=0, heads=None, out_scale=1.0, out_f32=False, pad_br_only=False, x_pix_stride=None, keep_cache=False):
    """Seeded operands, one dispatcher launch (cfg=-1, split_k=0), the fp32 reference, and every check but the dispatch assertion: values over the
    whole output, the sentinel behind it, statistics, a second identical call.  ``heads`` = (C, H, D, [(kind, DP, L, scale), ...]).
    ``keep_cache``: that launch runs with the decisions earlier problems left in ``ops._CFG_DECISIONS``; one more launch with the cache cleared
    (the cache is put back afterwards) must then run the same (cfg, split) and store the same bits.
    Returns (launches seen by the event hook, kind of statistics found)."""
    from imagdressing_amd import ops as ops_mod

    def cleared(call):
        kept = dict(ops_mod._CFG_DECISIONS)
        try:
            return _launch(ops_mod, call)
        finally:
            ops_mod._CFG_DECISIONS.clear()
            ops_mod._CFG_DECISIONS.update(kept)
    K = taps * Cin
    g = _gen(tag, dt)
    rows_in = B * Hin * Win if taps == 9 else M
    x = _randn(g, rows_in, Cin, dt=dt)
    w = _randn(g, N, K, scale=K ** -0.5, dt=dt)
    b = _randn(g, N) if bias else None
    base = ref_gemm(x.float(), w.float(), taps=taps, stride=stride, ups=ups, B=B, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, Cin=Cin, pad_br_only=pad_br_only)
    if b is not None:
        base += b
    xk = x
    geo = dict(M=M, N=N, Cin=Cin, taps=taps, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=stride, ups=bool(ups), bias=b, pad_br_only=pad_br_only)
    if x_pix_stride not in (None, Cin):         # the channels of a wider NHWC buffer
        xk = torch.full((rows_in, x_pix_stride), 7.0, dtype=dt, device=DEV)
        xk[:, :Cin] = x
        geo.update(x_pix_stride=x_pix_stride)
    what = f"{tag} [{str(dt).split('.')[-1]}]"
    if heads is not None:
        Cc, H, D, dests = heads
        HW = M // B
        assert N == len(dests) * Cc and Cc == H * D and not (res or rowvec or act or out_f32), what

        def call():
            bufs = [torch.zeros((B, H, L, DP) if kind == 0 else (B, H, DP, L), dtype=dt, device=DEV) for kind, DP, L, _ in dests]
            ops.conv_gemm(xk, w, heads=dict(C=Cc, H=H, D=D, dests=[(t, kind, DP, L, sc) for t, (kind, DP, L, sc) in zip(bufs, dests)]), **geo)
            return bufs
        bufs, seen = _launch(ops_mod, call, keep_cache)
        ref = base.view(B, HW, len(dests), H, D)
        for j, (t, (kind, DP, L, sc)) in enumerate(zip(bufs, dests)):
            if kind == 0:       # [B, H, L, DP] rows (Q / K)
                assert_close(t[:, :, :HW, :D], sc * ref[:, :, j].permute(0, 2, 1, 3), atol=TOL[dt], rtol=TOL[dt], what=f"{what} dest {j} (rows)")
                pads = (t[:, :, :, D:], t[:, :, HW:, :])
            else:               # [B, H, DP, L] (V^T)
                assert_close(t[:, :, :D, :HW], sc * ref[:, :, j].permute(0, 2, 3, 1), atol=TOL[dt], rtol=TOL[dt], what=f"{what} dest {j} (transposed)")
                pads = (t[:, :, D:, :], t[:, :, :, HW:])
            assert all(pz.numel() == 0 or float(pz.abs().max()) == 0.0 for pz in pads), f"{what}: dest {j}: the padding around the {HW} x {D} block was written"
        assert all(torch.equal(u, v) for u, v in zip(bufs, call())), f"{what}: second call differs"
        if keep_cache:
            bufs_c, seen_c = cleared(call)
            assert seen_c == seen, f"{what}: {seen} launched with the decision cache kept, {seen_c} with it cleared"
            assert all(torch.equal(u, v) for u, v in zip(bufs, bufs_c)), f"{what}: the launch with the decision cache kept stored other bits"
        return seen, "none"
    kw = dict(geo, act=act, out_scale=out_scale, out_f32=out_f32)
    ref = base
    if rowvec:
        rv = _randn(g, N) if rowvec_shared else _randn(g, B, N)
        kw.update(rowvec=rv, rowvec_stride=0 if rowvec_shared else N)
        ref = (ref.view(B, -1, N) + (rv[None, None, :] if rowvec_shared else rv[:, None, :])).view(M, N)
    if out_scale != 1.0:
        ref = ref * out_scale
    if res:
        rr = res_rows or M
        r = _randn(g, rr, N, dt=dt)
        kw.update(res=r)
        ref = ref + r.float().repeat(M // rr, 1)
    ref = _act(ops, act, ref)
    n_out = ref.shape[1]
    odt = torch.float32 if out_f32 else dt

    def call():
        buf = torch.full((M + 64, n_out), SENTINEL, dtype=odt, device=DEV)
        out = ops.conv_gemm(xk, w, out=buf[:M], gn_stats_groups=gn_groups, **kw)
        return out, buf
    (out, buf), seen = _launch(ops_mod, call, keep_cache)
    assert out.data_ptr() == buf.data_ptr() and out.dtype == odt
    assert_close(out, ref, atol=TOL[dt], rtol=TOL[dt], what=what)
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows behind the output were written"
    stats = "none"
    if gn_groups:
        stats = _check_stats(out, B, Hout * Wout, N, seen[0][2] if len(seen) == 1 else 1, what)
    out2, _ = call()
    assert torch.equal(out, out2), f"{what}: second call differs"
    if keep_cache:
        (out_c, _), seen_c = cleared(call)
        assert seen_c == seen, f"{what}: {seen} launched with the decision cache kept, {seen_c} with it cleared"
        assert torch.equal(out, out_c), f"{what}: the launch with the decision cache kept stored other bits"
    return seen, stats


def run_case(ops, c, dt):
    kw = dict(rowvec=c.rowvec, gn_groups=c.gn_groups)
    if c.form == "geglu":
        kw = dict(act=ops.ACT_GEGLU, res=False)         # (the library refuses a residual behind GEGLU; the product passes none)
    elif c.form == "heads":         # Q (with a scale), K, V^T in the attention layouts, as test_row_qkv / test_gemm_dma_head_split build them
        D, HW = c.K // HEADS, c.M // c.B
        try:
            DPK, DPV = ops.attn_padded_dims(D)
        except ops.L.ImdError:      # a head dim no attention kernel has (1024 / 8 = 128): the epilogue itself takes any layout, so unpadded rows and 64-padded V^T rows
            DPK, DPV = D, ops.pad64(D)
        kw = dict(res=False, heads=(c.K, HEADS, D, [(0, DPK, HW, Q_SCALE), (0, DPK, HW, 1.0), (1, DPV, ops.pad64(HW), 1.0)]))
    seen, stats = run_problem(ops, dt, c.id, M=c.M, N=c.N, Cin=c.Cin, taps=c.taps, stride=c.stride, ups=c.ups, B=c.B, Hin=c.Hin, Win=c.Win,
                              Hout=c.Hout, Wout=c.Wout, **kw)
    hook_key = f"{c.M},{c.N},{c.K},{c.taps},{c.stride},{c.ups}|{c.Hout}x{c.Wout}"
    assert len(seen) == 1 and seen[0][0] == hook_key, f"{c.id}: expected one launch of {hook_key}, the hook saw {seen}"
    launched = seen[0][1:]
    tabulated = launched == (c.table_cfg, c.table_split)
    RECORDS[(str(dt).split(".")[-1], c.id)] = dict(launched=launched, tabulated=tabulated, stats=stats)
    if c.form == "split" and not c.plain:       # linear and geometry-keyed entries: the tabulated kernel must take the problem it was timed on
        if c.key in EXPECTED_FALLBACKS:
            assert not tabulated and launched[0] != 15, f"{c.id}: the plain form cannot run on tile config 15, yet {launched} ran"
        else:
            assert tabulated, f"{c.id}: the table names (cfg, split) = {(c.table_cfg, c.table_split)}, the dispatcher launched {launched}"
    return launched


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_table_entry_bf16(ops, case):
    run_case(ops, case, bf16)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_table_entry_fp16(ops, case):
    """fp16 runs other template instantiations of every kernel: every case again (the whole module takes under a minute on an MI355X)"""
    run_case(ops, case, f16)


# ------------------------------------------------------------------------------------------
# the shapes the table does not hold: one denoising step of every benchmarked workload, traced
# ------------------------------------------------------------------------------------------
WORKLOADS = {
    "configs[1] 512x512 batch 4": dict(config=1, batch=4),
    "configs[1] 512x640 batch 1": dict(config=1, batch=1, width=512, height=640),
    "four requests in one call": dict(config=1, batch=1, requests=4),
    "configs[2] batch 8": dict(config=3, batch=8),
    "configs[4] 768x576 batch 4": dict(config=5, batch=4),
}
# full width, off the benchmarked geometries (tests/geometry_cases.py): the table was timed on none of these maps
GEOMETRY_WORKLOADS = {f"configs[1] latent {c.id}": workload_kwargs(c) for c in GEOMETRY_CASES}
WORKLOADS.update(GEOMETRY_WORKLOADS)
CACHE_KEPT_WORKLOADS = ("configs[1] latent 24x40 x3", "configs[1] latent 8x8")
CASE_KEYS = {c.key for c in CASES}
TRACES = {}             # workload -> (conv_gemm problems, attention launches) of one denoising step; tests/test_geometry_gpu.py replays the attention launches


def _configs_module():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "configs.py")
    spec = importlib.util.spec_from_file_location("imd_tools_configs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trace(ops_mod, config, batch, width=512, height=512, requests=0, garment=None):
    """One denoising step of a full-width random-weight pipeline with ``ops.GEMM_TRACE`` on and ``ops.attention`` recorded (shapes and flags only:
    ``GEMM_TRACE`` does not see attention launches); the pipeline is gone when this returns.  ``garment`` = (h, w): a garment latent of that size
    instead of the generation size.  -> (conv_gemm problems, attention launches)"""
    import gc
    dev = torch.device("cuda", 0)
    pipe, kw = _configs_module().build(config, dev, bf16, batch, steps=1, width=width, height=height)
    if garment is not None:
        kw["ref_image_latents"] = torch.randn(1, 4, *garment, generator=torch.Generator().manual_seed(78)).to(dev)
    if requests:        # R distinct (garment, prompt, latent, guidance, image scale) requests, as tests/test_multi_request_gpu.py::_Requests builds the call
        g = torch.Generator().manual_seed(77)
        rep = lambda t: (t.repeat(requests, *([1] * (t.dim() - 1))).float().cpu() + 0.1 * torch.randn(requests, *t.shape[1:], generator=g)).to(device=t.device, dtype=t.dtype)      # noqa: E731
        for name in ("prompt_embeds", "negative_prompt_embeds", "ref_clip_hidden_states", "ref_image_latents", "latents"):
            kw[name] = rep(kw[name])
        kw.update(guidance_scale=[5.0, 7.5, 9.0, 6.0][:requests], image_scale=[1.0, 0.6, 1.3, 0.8][:requests], num_images_per_prompt=1)
    attn = []
    real_attention = ops_mod.attention

    def recording_attention(q, k1, v1t, out, *, B, H, N, D, L1, L1P, kv1_bdiv=1, k2=None, v2t=None, scale2=None, L2=0, L2P=0, kv2_bdiv=1, out_ld=None,
                            causal=False, k_pad_one=False, proj=None, out_dup=None, phase2_rows=0):
        hybrid = k2 is not None and scale2 is not None
        attn.append(dict(B=B, H=H, N=N, D=D, L1=L1, L1P=L1P, kv1_bdiv=kv1_bdiv, L2=L2 if hybrid else 0, L2P=L2P if hybrid else 0, kv2_bdiv=kv2_bdiv if hybrid else 1,
                         scale2_rows=tuple(i for i, v in enumerate(scale2.tolist()) if v != 0.0) if hybrid else (), k_pad_one=bool(k_pad_one),
                         out_dup=out_dup is not None, phase2_rows=int(phase2_rows), causal=bool(causal), proj=proj is not None, out_ld=out_ld,
                         Bk1=k1.shape[0], Bk2=k2.shape[0] if hybrid else 0, dtype=str(q.dtype)))
        return real_attention(q, k1, v1t, out, B=B, H=H, N=N, D=D, L1=L1, L1P=L1P, kv1_bdiv=kv1_bdiv, k2=k2, v2t=v2t, scale2=scale2, L2=L2, L2P=L2P,
                              kv2_bdiv=kv2_bdiv, out_ld=out_ld, causal=causal, k_pad_one=k_pad_one, proj=proj, out_dup=out_dup, phase2_rows=phase2_rows)
    prev = ops_mod.GEMM_TRACE
    ops_mod.GEMM_TRACE = []
    ops_mod.attention = recording_attention
    try:
        with torch.no_grad():
            pipe(**kw)
        torch.cuda.synchronize()
        tr = ops_mod.GEMM_TRACE
    finally:
        ops_mod.GEMM_TRACE = prev
        ops_mod.attention = real_attention
    del pipe, kw
    gc.collect()
    ops_mod.clear_workspaces()
    torch.cuda.empty_cache()
    return tr, attn


def traced(ops_mod, workload):
    """The trace of a workload, taken once per session."""
    if workload not in TRACES:
        TRACES[workload] = _trace(ops_mod, **WORKLOADS[workload])
    return TRACES[workload]


def _problem_id(t):
    h = t["heads"]
    hs = "" if h is None else f" heads {h['H']}x{h['D']} kinds {[d[1] for d in h['dests']]}"
    epi = "+".join(n for n in ("bias", "rowvec", "res") if t[n]) or "bare"
    return (f"{t['M']},{t['N']},{t['K']},{t['taps']},{t['stride']},{t['ups']}|{t['Hout']}x{t['Wout']} {epi} act {t['act']}{hs}"
            + (" f32" if t["out_f32"] else "") + (" pad_br" if t["pad_br_only"] else "") + (f" scale {t['out_scale']:g}" if t["out_scale"] != 1.0 else "")
            + (f" gn_stats {t['gn_stats_groups']}" if t["gn_stats_groups"] else "") + (f" res_rows {t['res_rows']}" if t["res_rows"] else "")
            + (f" xps {t['x_pix_stride']}" if t["x_pix_stride"] != t["Cin"] else "") + ("" if t["rowvec_stride"] or not t["rowvec"] else " shared rowvec"))


def _distinct_problems(tr):
    distinct = {}
    for t in tr:
        if t["gn"]:             # GroupNorm of the input inside the conv: the caller names the kernel, nothing is dispatched (own tests)
            continue
        distinct.setdefault(_problem_id(t), t)
    return distinct


def _replay(ops, workload, pid, t, keep_cache=False):
    """One traced problem standalone in its traced geometry and epilogue (``run_problem``) -> the launches the event hook saw."""
    heads = None
    if t["heads"] is not None:
        h = t["heads"]
        assert all(d[0] for d in h["dests"]), f"{pid}: a head-split launch with an absent destination"
        heads = (h["C"], h["H"], h["D"], [(kind, DP, L, sc) for _, kind, DP, L, sc in h["dests"]])
    n_out = t["N"] // 2 if t["act"] == ops.ACT_GEGLU else t["N"]
    assert (heads is not None or t["out_ld"] == n_out) and (not t["res"] or t["res_ld"] == t["N"]), f"{pid}: a strided output or residual, which this replay does not build"
    seen, _ = run_problem(ops, bf16, f"{workload}: {pid}", M=t["M"], N=t["N"], Cin=t["Cin"], taps=t["taps"], stride=t["stride"], ups=t["ups"],
                          B=t["M"] // (t["Hout"] * t["Wout"]), Hin=t["Hin"], Win=t["Win"], Hout=t["Hout"], Wout=t["Wout"], bias=t["bias"], res=t["res"],
                          res_rows=t["res_rows"], rowvec=t["rowvec"], rowvec_shared=t["rowvec_stride"] == 0, act=t["act"], gn_groups=t["gn_stats_groups"],
                          heads=heads, out_scale=t["out_scale"], out_f32=t["out_f32"], pad_br_only=t["pad_br_only"], x_pix_stride=t["x_pix_stride"],
                          keep_cache=keep_cache)
    return seen


@pytest.mark.parametrize("workload", list(WORKLOADS))
def test_untabulated_problems_of_a_workload(ops, workload):
    """Every problem one denoising step launches through the dispatcher is either a table entry (then the sweep above has a case for its key)
    or is replayed standalone in its traced geometry and epilogue: values over the whole output, sentinel, second call.
    The workloads off the benchmarked geometries replay their table hits as well: the sweep above launches an entry on the map it was timed on,
    here the same key arrives from another map (or another image count), and whatever (cfg, split) runs must be one the library's own
    ``*_supported`` query accepts for that problem."""
    tr, _ = traced(ops, workload)
    assert tr, "the workload launched nothing through ops.conv_gemm"
    foreign = workload in GEOMETRY_WORKLOADS
    distinct = _distinct_problems(tr)
    hits, misses, failures, ran = [], [], [], {}
    n_refused = len(REFUSED)
    for pid, t in distinct.items():
        key = lookup_key(TABLE, t["M"], t["N"], t["K"], t["taps"], t["stride"], t["ups"], t["Hout"], t["Wout"])
        if key is not None:
            assert key in CASE_KEYS, f"{workload}: table entry {key} is launched by the product but by no case of the sweep"
            hits.append(pid)
            if not foreign:
                continue
        else:
            misses.append(pid)
        try:
            seen = _replay(ops, workload, pid, t)
            assert len(seen) == 1, f"{workload}: {pid}: expected one launch, the hook saw {seen}"
            ran[pid] = seen[0][1:]
        except AssertionError as e:
            failures.append(str(e))
    MISSES[workload] = dict(launches=len(tr), distinct=len(distinct), tabulated=len(hits), misses=misses, foreign_hits=hits if foreign else [], ran=ran)
    assert not failures, f"{len(failures)} of {len(ran) + len(failures)} replayed problems of {workload} failed:\n" + "\n".join(failures)
    assert len(REFUSED) == n_refused, f"{workload}: launched although the tile config's *_supported query refuses the problem: {REFUSED[n_refused:]}"


@pytest.mark.parametrize("workload", CACHE_KEPT_WORKLOADS)
def test_decision_cache_kept_across_the_problems_of_a_workload(ops, workload):
    """``ops._CFG_DECISIONS`` remembers (cfg, split) per problem description, and that description leaves out ``gn`` / ``gn_in`` / ``gn_out`` /
    ``gn_stats_groups`` / ``res_rows`` / ``rowvec_stride``; every replay above clears it first.  Here the distinct problems of two workloads run
    back to back (the second workload finds the first one's decisions) with the cache KEPT: each problem must launch the (cfg, split) it launches with
    a cleared cache, store the same bits, meet the same value / sentinel / statistics checks, and never run a tile config whose ``*_supported``
    query refuses it."""
    from imagdressing_amd import ops as ops_mod
    if not CACHE_KEPT:
        ops_mod._CFG_DECISIONS.clear()
    tr, _ = traced(ops, workload)
    distinct = _distinct_problems(tr)
    failures, n_refused, hits_before = [], len(REFUSED), len(ops_mod._CFG_DECISIONS)
    for pid, t in distinct.items():
        try:
            _replay(ops, workload, pid, t, keep_cache=True)
        except AssertionError as e:
            failures.append(str(e))
    CACHE_KEPT[workload] = dict(problems=len(distinct), decisions_before=hits_before, decisions_after=len(ops_mod._CFG_DECISIONS))
    assert len(ops_mod._CFG_DECISIONS) > hits_before, "the replay left no decision in the cache: it is not exercised"
    assert not failures, f"{len(failures)} of {len(distinct)} problems of {workload} differ with the decision cache kept:\n" + "\n".join(failures)
    assert len(REFUSED) == n_refused, f"{workload}: launched although the tile config's *_supported query refuses the problem: {REFUSED[n_refused:]}"


def test_zz_summary(ops):
    """What the module did, for the pull-request description (``pytest -rA`` shows it)."""
    from collections import Counter
    lines = [f"dispatch sweep: {len(TABLE)} table entries, {len(CASES)} cases per form: {dict(Counter(c.form for c in CASES))}"]
    for dname in ("bfloat16", "float16"):
        recs = {cid: r for (d, cid), r in RECORDS.items() if d == dname}
        if not recs:
            lines.append(f"{dname}: no case ran")
            continue
        lines.append(f"{dname}: {len(recs)} of {len(CASES)} cases ran")
        per = Counter(r["launched"] for r in recs.values())
        lines.append("  cases per launched (cfg, split): " + ", ".join(f"{k}: {n}" for k, n in sorted(per.items())))
        lines.append("  GroupNorm statistics checked: " + str(dict(Counter(r["stats"] for r in recs.values()))))
        byid = {c.id: c for c in CASES}
        for name, sel in (("GEGLU", lambda c: c.form == "geglu"), ("head-split", lambda c: c.form == "heads"), ("plain-key", lambda c: c.plain),
                          ("linear / geometry-keyed splittable", lambda c: c.form == "split" and not c.plain)):
            ran = [cid for cid in recs if sel(byid[cid])]
            back = [f"{byid[cid].key} -> {recs[cid]['launched']}" for cid in ran if not recs[cid]["tabulated"]]
            lines.append(f"  {name}: {len(ran) - len(back)} ran the tabulated kernel, {len(back)} fell back to the heuristic" + (": " + "; ".join(back) if back else ""))
    for wl, m in MISSES.items():
        if wl in GEOMETRY_WORKLOADS:
            lines.append(f"{wl}: {m['launches']} launches, {m['distinct']} distinct problems, {len(m['foreign_hits'])} table hits on a foreign map, {len(m['misses'])} table misses, "
                         f"{len(m['ran'])} replayed; (cfg, split) per problem:" + "".join(f"\n    {p} -> {m['ran'].get(p)}" + (" [table hit]" if p in m["foreign_hits"] else "")
                                                                                       for p in m["foreign_hits"] + m["misses"]))
            continue
        lines.append(f"{wl}: {m['launches']} launches, {m['distinct']} distinct problems, {m['tabulated']} tabulated, {len(m['misses'])} replayed table misses"
                     + ("".join("\n    " + p for p in m["misses"])))
    for wl, m in CACHE_KEPT.items():
        lines.append(f"decision cache kept, {wl}: {m['problems']} problems, {m['decisions_before']} -> {m['decisions_after']} remembered decisions")
    for wl, (_, at) in TRACES.items():
        if wl in GEOMETRY_WORKLOADS:
            lines.append(f"{wl}: {len(at)} attention launches, {len({tuple(sorted((k, str(v)) for k, v in a.items())) for a in at})} distinct")
    lines.append(f"launches of a tile config whose own *_supported query refuses the problem: {len(REFUSED)}" + "".join(f"\n    {r}" for r in REFUSED[:20]))
    lines.append(f"wall time of the module: {time.time() - T0[0]:.0f} s")
    print("\n".join(lines))
    ran = {cid for (d, cid) in RECORDS if d == "bfloat16"}
    if len(ran) > len(CASES) // 2:          # (a whole run, not a -k selection: no entry of the table may have gone unlaunched)
        unlaunched = sorted(set(TABLE) - {c.key for c in CASES if c.id in ran})
        assert not unlaunched, f"table entries no bf16 case launched: {unlaunched}"
