"""imd_attention at head dim 512 (attention_d512.hip): the VAE mid block's attention as one flash launch.

1. The exact cases of tests/attention_d512_cases.py (integer-valued heads, softmax2(S) V known to the last place; preconditions and the
   sensitivity of the comparison: tests/test_attention_d512_inputs.py) in both element types, 16449 keys included.  Tolerance: one unit in the
   last place plus 2^-20 max|V|, derived in tests/attention_exact_cases.py.  `out` is a window of a sentinel-filled buffer with two guard rows in
   front of the first and behind the last batch entry and, on every second case, out_ld = H 512 + 8.
2. Gaussian q / k / v against the fp32 sdpa of oracle/processors.py at the bar of tests/test_kernels_gpu.py::test_attention.
3. One launch at B = 2 equals two launches at B = 1, bit for bit.
4. Every parameter the kernel does not take is refused by name and nothing is written."""
import ctypes as C
import math

import pytest
import torch

from tests import attention_d512_cases as dc
from tests import attention_exact_cases as ac

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
SENTINEL = -976.0            # representable in both types, far outside every expectation, finite
GUARD_ROWS, GUARD_COLS = 2, 8
D = 512


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops as o
    return o


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_padded_dims_match_the_library(ops):
    assert ops.attn_padded_dims(D) == ac.padded_dims(D) == (D, D)


@pytest.mark.parametrize("idx", range(len(dc.CASES)), ids=[c.name for c in dc.CASES])
@DTS
def test_exact_cases(ops, idx, dt):
    case = dc.CASES[idx]
    exp = ac.expectation(case, dt)
    d = {k: (None if v is None else v.to("cuda")) for k, v in ac.pack(case, dt).items()}
    rows, Cc = case.B * case.N, case.H * D
    ld = Cc + (GUARD_COLS if idx % 2 else 0)
    full = torch.full((rows + 2 * GUARD_ROWS, ld), SENTINEL, dtype=dt, device="cuda")
    ops.attention(d["q"], d["k1"], d["v1t"], full[GUARD_ROWS:GUARD_ROWS + rows], B=case.B, H=case.H, N=case.N, D=D, L1=case.L1,
                  L1P=ac.pad64(case.L1), kv1_bdiv=case.bdiv1, out_ld=ld)
    torch.cuda.synchronize()
    full = full.cpu()
    bits = full.view(torch.int16)
    fresh = torch.full((1,), SENTINEL, dtype=dt).view(torch.int16).item()
    assert bool((bits[:GUARD_ROWS] == fresh).all()), f"{case.name}: rows in front of the first batch entry were written"
    assert bool((bits[GUARD_ROWS + rows:] == fresh).all()), f"{case.name}: rows behind query row N - 1 of the last batch entry were written"
    assert bool((bits[:, Cc:] == fresh).all()), f"{case.name}: columns at or beyond H * D = {Cc} were written"
    got = full[GUARD_ROWS:GUARD_ROWS + rows, :Cc]
    assert bool(torch.isfinite(got.float()).all()), f"{case.name}: {int((~torch.isfinite(got.float())).sum())} written elements are not finite"
    ac.assert_exact(got, exp, case.name)


def heads(x, H, scale=1.0, dt=None):
    """[B, L, H * D] -> [B, H, L, D]"""
    B, L, _ = x.shape
    return (x.float() * scale).view(B, L, H, D).permute(0, 2, 1, 3).contiguous().to(dt)


def heads_t(x, H, LP, dt):
    """[B, L, H * D] -> V^T [B, H, D, LP], zero padded"""
    B, L, _ = x.shape
    out = torch.zeros(B, H, D, LP, dtype=dt)
    out[..., :L] = x.view(B, L, H, D).permute(0, 2, 3, 1)
    return out


def run(ops, q, k, v, H, dt, B=None):
    """q [B, N, H D], k / v [B, L, H D] of `dt` on the CPU -> out [B, N, H D] on the GPU"""
    B = q.shape[0] if B is None else B
    N, L = q.shape[1], k.shape[1]
    out = torch.empty(B, N, H * D, dtype=dt, device="cuda")
    ops.attention(heads(q, H, D ** -0.5 * math.log2(math.e), dt).cuda(), heads(k, H, dt=dt).cuda(), heads_t(v, H, ac.pad64(L), dt).cuda(), out,
                  B=B, H=H, N=N, D=D, L1=L, L1P=ac.pad64(L))
    return out


@pytest.mark.parametrize("B,H,N,L1", [(2, 1, 200, 200), (1, 2, 70, 273), (1, 1, 1024, 1024)])
@DTS
def test_gaussian_parity(ops, B, H, N, L1, dt):
    from oracle.processors import sdpa
    from tests.test_kernels_gpu import assert_close
    q, k, v = rnd(1, B, N, H * D).to(dt), rnd(2, B, L1, H * D).to(dt), rnd(3, B, L1, H * D).to(dt)
    ref = sdpa(q.float(), k.float(), v.float(), H)
    assert_close(run(ops, q, k, v, H, dt), ref, atol=1e-2, rtol=1e-2, what=f"attention D=512 B={B} H={H} N={N} L1={L1}")


@DTS
def test_batch_invariance(ops, dt):
    """What a batch entry gets does not depend on what else is in the launch."""
    N = 320
    q, k, v = rnd(4, 2, N, D).to(dt), rnd(5, 2, N, D).to(dt), rnd(6, 2, N, D).to(dt)
    assert not torch.equal(q[0], q[1])
    both = run(ops, q, k, v, 1, dt)
    for b in range(2):
        one = run(ops, q[b:b + 1], k[b:b + 1], v[b:b + 1], 1, dt)
        assert torch.equal(both[b].view(torch.int16), one[0].view(torch.int16)), f"batch entry {b} differs between the B = 2 and the B = 1 launch"
    assert bool(torch.isfinite(both.float()).all())


REFUSED = ("k2", "scale2", "causal", "proj_w", "out_dup", "phase2_out", "k_pad_one")


@pytest.mark.parametrize("what", REFUSED)
def test_refusals(ops, what):
    """The parameter block is filled by hand (ops.attention drops some of these where the library says it cannot take them)."""
    L = ops.L
    dt = torch.float16
    B, N = 1, 64
    q = torch.zeros(B, 1, N, D, dtype=dt, device="cuda")
    vt = torch.zeros(B, 1, D, N, dtype=dt, device="cuda")
    out = torch.full((B, N, D), SENTINEL, dtype=dt, device="cuda")
    other = torch.full((B, N, D), SENTINEL, dtype=torch.float32, device="cuda")          # whatever the refused pointer points at
    p = L.AttnParams()
    p.dtype = ops._code(q, "q")
    p.q, p.k1, p.v1t, p.out = q.data_ptr(), q.data_ptr(), vt.data_ptr(), out.data_ptr()
    p.B, p.H, p.N, p.D, p.L1, p.L1P, p.kv1_bdiv, p.kv2_bdiv, p.out_ld = B, 1, N, D, N, N, 1, 1, D
    if what == "k2":
        p.k2, p.v2t, p.L2, p.L2P = q.data_ptr(), vt.data_ptr(), N, N
    elif what == "scale2":
        p.scale2 = other.data_ptr()
    elif what == "causal":
        p.causal = 1
    elif what == "proj_w":
        p.proj_w, p.proj_out, p.proj_counters, p.proj_out_ld = q.data_ptr(), other.data_ptr(), other.data_ptr(), D
    elif what == "out_dup":
        p.out_dup = other.data_ptr()
    elif what == "phase2_out":
        p.phase2_out, p.phase2_rows = other.data_ptr(), 1
    elif what == "k_pad_one":
        p.k_pad_one = 1
    rc = L.load().imd_attention(C.byref(p), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0, f"{what} was accepted at head dim 512"
    msg = L.load().imd_last_error().decode()
    assert what in msg and "512" in msg, msg
    with pytest.raises(L.ImdError):
        L.check(rc)
    assert bool((out == SENTINEL).all()) and bool((other == SENTINEL).all()), f"{what}: refused, but something was written"
