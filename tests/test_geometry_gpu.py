"""The attention launches of the full-width workloads OFF the benchmarked geometries (tests/geometry_cases.py), replayed standalone.

``ops.GEMM_TRACE`` does not see attention launches, so tests/test_dispatch_sweep_gpu.py::_trace records them (shapes and flags only) during the
same denoising step it traces the GEMMs of.  Every distinct launch is rebuilt here from seeded operands in the kernels' layouts and compared with
``oracle.processors.sdpa`` on the same rounded inputs, the way tests/test_kernels_gpu.py::test_attention does; the two launch forms the processors
choose by geometry are checked against their plain forms bit for bit.  ``pytest -rA`` shows the distinct problems per workload.

What the bars notice at these shapes (faults planted in the reference, both element types, every distinct problem of the 8x8, 16x32 and 24x24 /
garment 16x24 workloads): a dropped last key, a temperature off by 5 % and V shifted by one key each fail every problem but the four with a single
key, where softmax is 1 whatever the scores are."""
import math

import pytest
import torch

from tests.test_dispatch_sweep_gpu import GEOMETRY_WORKLOADS, traced
from tests.test_kernels_gpu import assert_close, ref_attn, rnd, to_heads, to_heads_t

pytestmark = pytest.mark.gpu

# scores of std 2: rows peaked enough for the outputs to be O(0.1 .. 1), where the relative part of the bar bites.  (At that spread the kernel's Q operand
# must be modelled as it is stored -- rounded AFTER the d^-1/2 log2(e) scaling: a reference on the unscaled rounded Q is off by 2^-9 of every score.)
Q_STD = 2.0
REPLAYED = {}           # (dtype name, problem) -> workload that replayed it first
SUMMARY = {}            # workload -> [problem description, ...]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def _describe(a):
    return (f"B {a['B']} H {a['H']} N {a['N']} D {a['D']} L1 {a['L1']}/{a['L1P']} bdiv {a['kv1_bdiv']}"
            + (f" L2 {a['L2']}/{a['L2P']} bdiv {a['kv2_bdiv']} garment rows {list(a['scale2_rows'])}" if a["L2"] else "")
            + (" k_pad_one" if a["k_pad_one"] else "") + (" out_dup" if a["out_dup"] else "") + (f" phase2_rows {a['phase2_rows']}" if a["phase2_rows"] else ""))


def _replay(ops, a, dt):
    """One recorded launch: seeded [B, L, C] operands -> the kernels' head layouts (K pad column 1.0 where ``k_pad_one``) -> ``ops.attention`` with the
    recorded shapes and flags, against sdpa in fp32 on the same rounded operands (first phase rounded to the element type before the add)."""
    assert not (a["causal"] or a["proj"] or a["out_ld"] not in (None, a["H"] * a["D"])), f"a launch form this replay does not build: {a}"
    B, H, N, D, L1, L2 = a["B"], a["H"], a["N"], a["D"], a["L1"], a["L2"]
    Cc = H * D
    dpk, dpv = ops.attn_padded_dims(D)
    assert a["L1P"] == ops.pad64(L1) and a["L2P"] == (ops.pad64(L2) if L2 else 0), a
    # query b reads K / V rows b // bdiv; the second key set is read by the rows with a non-zero scale2 only (the cond rows of a CFG batch)
    assert (B - 1) // a["kv1_bdiv"] < a["Bk1"] and (not L2 or max(a["scale2_rows"], default=0) // a["kv2_bdiv"] < a["Bk2"]), f"batch divisors that index past the K / V rows: {a}"

    def kbuf(x):
        h = to_heads(x, H, dpk, dt=dt)
        if a["k_pad_one"] and dpk > D:      # as ops.k_buffer: the pad column exists for head dim 40 only
            h[..., D] = 1.0
        return h.cuda()

    def rows(x, bdiv):          # [Bk, L, C] -> the K / V rows each of the B queries reads (rows past the end belong to queries that do not read the set)
        return x[(torch.arange(B) // bdiv).clamp(max=x.shape[0] - 1)]
    qscale = D ** -0.5 * math.log2(math.e)
    qh = to_heads((rnd(1, B, N, Cc) * Q_STD).to(dt), H, dpk, qscale, dt=dt)
    # the kernel's Q operand carries d^-1/2 log2(e) and is rounded WITH it: the reference reads the same rounded values, scaled back
    q = (qh[..., :D].float() / qscale).transpose(1, 2).reshape(B, N, Cc)
    k1, v1 = rnd(2, a["Bk1"], L1, Cc).to(dt), rnd(3, a["Bk1"], L1, Cc).to(dt)
    ref1 = ref_attn(q, rows(k1, a["kv1_bdiv"]), rows(v1, a["kv1_bdiv"]), H)
    ref = ref1
    kw = {}
    if L2:
        k2, v2 = rnd(4, a["Bk2"], L2, Cc).to(dt), rnd(5, a["Bk2"], L2, Cc).to(dt)
        s2 = torch.zeros(B)
        s2[list(a["scale2_rows"])] = torch.tensor([0.9, 1.0, 0.6, 1.3] * B)[:len(a["scale2_rows"])]
        r2 = ref_attn(q, rows(k2, a["kv2_bdiv"]), rows(v2, a["kv2_bdiv"]), H)
        ref = ref1.to(dt).float() + s2[:, None, None] * r2
        kw = dict(k2=kbuf(k2), v2t=to_heads_t(v2, H, dpv, a["L2P"], dt=dt).cuda(), scale2=s2.cuda(), L2=L2, L2P=a["L2P"], kv2_bdiv=a["kv2_bdiv"])
    qh = qh.cuda()
    k1h, v1t = kbuf(k1), to_heads_t(v1, H, dpv, a["L1P"], dt=dt).cuda()
    base = dict(B=B, H=H, N=N, D=D, L1=L1, L1P=a["L1P"], kv1_bdiv=a["kv1_bdiv"], k_pad_one=a["k_pad_one"])

    def launch(out, **more):
        ops.attention(qh, k1h, v1t, out, **base, **more)
        return out
    what = f"attention {_describe(a)} [{str(dt).split('.')[-1]}]"
    out = torch.empty(B, N, Cc, dtype=dt, device="cuda")
    dup = torch.empty_like(out) if a["out_dup"] else None
    launch(out, out_dup=dup, phase2_rows=a["phase2_rows"], **kw)
    assert torch.isfinite(out).all(), what
    if D == 40 and N >= 512:        # the software-pipelined head-dim-40 kernel: bars of test_attention_d40_kernel_variants
        assert_close(out, ref, atol=1e-2 if dt == torch.float16 else 2e-2, rtol=2e-2, what=what)
    else:                           # bars of test_attention
        assert_close(out, ref, atol=1e-2, rtol=1e-2, what=what)
    if a["out_dup"]:                # the duplicated first phase == a plain launch without the second key set, bit for bit
        assert ops.attention_dup_supported(H, N, D), f"{what}: out_dup recorded where attention_dup_supported says no"
        plain = launch(torch.empty_like(out))
        assert torch.equal(dup, plain), f"{what}: out_dup differs from the launch without a second key set"
        assert_close(dup, ref1, atol=1e-2 if dt == torch.float16 else 2e-2, rtol=2e-2, what=what + " (out_dup)")
    if a["phase2_rows"]:            # the phase-split launch == the one-workgroup form, bit for bit
        assert list(a["scale2_rows"]) == list(range(a["phase2_rows"])), f"{what}: phase2_rows promises garment rows [0, R)"
        one = launch(torch.empty_like(out), **kw)
        assert torch.equal(out, one), f"{what}: the phase-split launch differs from the one-workgroup form"
    assert torch.equal(out, launch(torch.empty_like(out), out_dup=None if dup is None else torch.empty_like(out), phase2_rows=a["phase2_rows"], **kw)), f"{what}: second call differs"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("workload", list(GEOMETRY_WORKLOADS))
def test_attention_launches_of_a_workload(ops, workload, dt):
    """Every distinct attention launch of one denoising step (self + garment hybrid attention of the 16 attn1 layers, text cross-attention of the 16
    attn2 layers, in both UNets), replayed in both element types.  A problem an earlier workload of the session already replayed is not run again."""
    _, attn = traced(ops, workload)
    assert attn, "the workload launched no attention"
    distinct = {}
    for a in attn:
        distinct.setdefault(_describe(a), a)
    SUMMARY[workload] = list(distinct)
    dname = str(dt).split(".")[-1]
    failures = []
    for pid, a in distinct.items():
        if REPLAYED.setdefault((dname, pid), workload) != workload:
            continue
        try:
            _replay(ops, a, dt)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(distinct)} attention problems of {workload} failed:\n" + "\n".join(failures)


def test_zz_attention_shapes_and_summary(ops):
    """The shapes the list was built to reach were really launched (a whole run only), and the distinct problems per workload for ``pytest -rA``."""
    for wl, pids in SUMMARY.items():
        print(f"{wl}: {len(pids)} distinct attention problems" + "".join("\n    " + p for p in pids))
    if set(SUMMARY) != set(GEOMETRY_WORKLOADS):
        return
    launched = [a for wl in GEOMETRY_WORKLOADS for a in traced(ops, wl)[1]]
    assert {1, 4, 9, 15, 36, 60, 512, 576, 960} <= {a["N"] for a in launched}, sorted({a["N"] for a in launched})
    assert {(6, 9), (24, 36), (96, 144), (384, 576)} <= {(a["L2"], a["N"]) for a in launched}
    assert any(a["out_dup"] for a in launched) and any(a["phase2_rows"] for a in launched)
