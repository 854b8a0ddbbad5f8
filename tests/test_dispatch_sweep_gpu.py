"""Every entry of the GEMM / conv tuning table, launched the way the product launches it (``ops.conv_gemm(cfg=-1, split_k=0)``: the
dispatcher reads ``gemm_tuning.json``) and compared over the WHOLE output with an fp32 computation written here from plain torch.

Per case (tests/dispatch_cases.py turns the table into cases): which kernel ran (one launch; its (tile config, K slices) against the
table's choice), values at the bar of tests/test_kernels_gpu.py, GroupNorm statistics where the launch hands them on, a sentinel tail
behind the output, and a second identical call.  The shapes the table does NOT hold are collected from one denoising step of each
benchmarked workload (``ops.GEMM_TRACE``) and replayed the same way.  The last test prints the module's summary (``-rA``)."""
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.dispatch_cases import HEADS, cases, load_table, lookup_key
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


def _launch(ops_mod, kwargs_fn):
    """One dispatcher call under the event hook, decision cache cleared: (result, [(key, cfg, split), ...] launches)."""
    hook = ops_mod.GEMM_EVENT_HOOK
    ops_mod._CFG_DECISIONS.clear()
    ops_mod.GEMM_EVENT_HOOK = {}
    try:
        r = kwargs_fn()
        seen = [k for k, ev in ops_mod.GEMM_EVENT_HOOK.items() for _ in ev]
    finally:
        ops_mod.GEMM_EVENT_HOOK = hook
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
                rowvec_shared=False, act=0, gn_groups=0, heads=None, out_scale=1.0, out_f32=False, pad_br_only=False, x_pix_stride=None):
    """Seeded operands, one dispatcher launch (cfg=-1, split_k=0), the fp32 reference, and every check but the dispatch assertion: values over the
    whole output, the sentinel behind it, statistics, a second identical call.  ``heads`` = (C, H, D, [(kind, DP, L, scale), ...]).
    Returns (launches seen by the event hook, kind of statistics found)."""
    from imagdressing_amd import ops as ops_mod
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
        bufs, seen = _launch(ops_mod, call)
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
    (out, buf), seen = _launch(ops_mod, call)
    assert out.data_ptr() == buf.data_ptr() and out.dtype == odt
    assert_close(out, ref, atol=TOL[dt], rtol=TOL[dt], what=what)
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows behind the output were written"
    stats = "none"
    if gn_groups:
        stats = _check_stats(out, B, Hout * Wout, N, seen[0][2] if len(seen) == 1 else 1, what)
    out2, _ = call()
    assert torch.equal(out, out2), f"{what}: second call differs"
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
CASE_KEYS = {c.key for c in CASES}


def _configs_module():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "configs.py")
    spec = importlib.util.spec_from_file_location("imd_tools_configs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trace(ops_mod, config, batch, width=512, height=512, requests=0):
    """One denoising step of a full-width random-weight pipeline with ``ops.GEMM_TRACE`` on; the pipeline is gone when this returns."""
    import gc
    dev = torch.device("cuda", 0)
    pipe, kw = _configs_module().build(config, dev, bf16, batch, steps=1, width=width, height=height)
    if requests:        # R distinct (garment, prompt, latent, guidance, image scale) requests, as tests/test_multi_request_gpu.py::_Requests builds the call
        g = torch.Generator().manual_seed(77)
        rep = lambda t: (t.repeat(requests, *([1] * (t.dim() - 1))).float().cpu() + 0.1 * torch.randn(requests, *t.shape[1:], generator=g)).to(device=t.device, dtype=t.dtype)      # noqa: E731
        for name in ("prompt_embeds", "negative_prompt_embeds", "ref_clip_hidden_states", "ref_image_latents", "latents"):
            kw[name] = rep(kw[name])
        kw.update(guidance_scale=[5.0, 7.5, 9.0, 6.0][:requests], image_scale=[1.0, 0.6, 1.3, 0.8][:requests], num_images_per_prompt=1)
    prev = ops_mod.GEMM_TRACE
    ops_mod.GEMM_TRACE = []
    try:
        with torch.no_grad():
            pipe(**kw)
        torch.cuda.synchronize()
        tr = ops_mod.GEMM_TRACE
    finally:
        ops_mod.GEMM_TRACE = prev
    del pipe, kw
    gc.collect()
    ops_mod.clear_workspaces()
    torch.cuda.empty_cache()
    return tr


def _problem_id(t):
    h = t["heads"]
    hs = "" if h is None else f" heads {h['H']}x{h['D']} kinds {[d[1] for d in h['dests']]}"
    epi = "+".join(n for n in ("bias", "rowvec", "res") if t[n]) or "bare"
    return (f"{t['M']},{t['N']},{t['K']},{t['taps']},{t['stride']},{t['ups']}|{t['Hout']}x{t['Wout']} {epi} act {t['act']}{hs}"
            + (" f32" if t["out_f32"] else "") + (" pad_br" if t["pad_br_only"] else "") + (f" scale {t['out_scale']:g}" if t["out_scale"] != 1.0 else "")
            + (f" gn_stats {t['gn_stats_groups']}" if t["gn_stats_groups"] else "") + (f" res_rows {t['res_rows']}" if t["res_rows"] else "")
            + (f" xps {t['x_pix_stride']}" if t["x_pix_stride"] != t["Cin"] else "") + ("" if t["rowvec_stride"] or not t["rowvec"] else " shared rowvec"))


@pytest.mark.parametrize("workload", list(WORKLOADS))
def test_untabulated_problems_of_a_workload(ops, workload):
    """Every problem one denoising step launches through the dispatcher is either a table entry (then the sweep above has a case for its key)
    or is replayed standalone in its traced geometry and epilogue: values over the whole output, sentinel, second call."""
    from imagdressing_amd import ops as ops_mod
    tr = _trace(ops_mod, **WORKLOADS[workload])
    assert tr, "the workload launched nothing through ops.conv_gemm"
    distinct = {}
    for t in tr:
        if t["gn"]:             # GroupNorm of the input inside the conv: the caller names the kernel, nothing is dispatched (own tests)
            continue
        distinct.setdefault(_problem_id(t), t)
    hits, misses, failures = 0, [], []
    for pid, t in distinct.items():
        key = lookup_key(TABLE, t["M"], t["N"], t["K"], t["taps"], t["stride"], t["ups"], t["Hout"], t["Wout"])
        if key is not None:
            assert key in CASE_KEYS, f"{workload}: table entry {key} is launched by the product but by no case of the sweep"
            hits += 1
            continue
        misses.append(pid)
        heads = None
        if t["heads"] is not None:
            h = t["heads"]
            assert all(d[0] for d in h["dests"]), f"{pid}: a head-split launch with an absent destination"
            heads = (h["C"], h["H"], h["D"], [(kind, DP, L, sc) for _, kind, DP, L, sc in h["dests"]])
        n_out = t["N"] // 2 if t["act"] == ops.ACT_GEGLU else t["N"]
        assert (heads is not None or t["out_ld"] == n_out) and (not t["res"] or t["res_ld"] == t["N"]), f"{pid}: a strided output or residual, which this replay does not build"
        try:
            run_problem(ops, bf16, f"{workload}: {pid}", M=t["M"], N=t["N"], Cin=t["Cin"], taps=t["taps"], stride=t["stride"], ups=t["ups"],
                        B=t["M"] // (t["Hout"] * t["Wout"]), Hin=t["Hin"], Win=t["Win"], Hout=t["Hout"], Wout=t["Wout"], bias=t["bias"], res=t["res"],
                        res_rows=t["res_rows"], rowvec=t["rowvec"], rowvec_shared=t["rowvec_stride"] == 0, act=t["act"], gn_groups=t["gn_stats_groups"],
                        heads=heads, out_scale=t["out_scale"], out_f32=t["out_f32"], pad_br_only=t["pad_br_only"], x_pix_stride=t["x_pix_stride"])
        except AssertionError as e:
            failures.append(str(e))
    MISSES[workload] = dict(launches=len(tr), distinct=len(distinct), tabulated=hits, misses=misses)
    assert not failures, f"{len(failures)} of {len(misses)} untabulated problems of {workload} failed:\n" + "\n".join(failures)


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
        lines.append(f"{wl}: {m['launches']} launches, {m['distinct']} distinct problems, {m['tabulated']} tabulated, {len(m['misses'])} replayed table misses"
                     + ("".join("\n    " + p for p in m["misses"])))
    lines.append(f"wall time of the module: {time.time() - T0[0]:.0f} s")
    print("\n".join(lines))
    ran = {cid for (d, cid) in RECORDS if d == "bfloat16"}
    if len(ran) > len(CASES) // 2:          # (a whole run, not a -k selection: no entry of the table may have gone unlaunched)
        unlaunched = sorted(set(TABLE) - {c.key for c in CASES if c.id in ran})
        assert not unlaunched, f"table entries no bf16 case launched: {unlaunched}"
