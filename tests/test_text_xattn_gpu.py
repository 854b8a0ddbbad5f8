"""One-launch text cross-attention of the 64x64 level (csrc/row_xattn.hip, ops.text_xattn) against an fp64 evaluation of

    out = x + b_o + W_o concat_h softmax(q_h K_h^T / sqrt(d)) V_h,     q = LN(x) W_q'^T + b_q'

on the same 16-bit inputs.  The bar is the three-launch path's own error on the same inputs (ops.FUSED_XATTN off: norm2 + to_q,
attention, to_out + residual): both paths round at the same four points (q, P, O, out) and differ only in fp32 summation order
and in the softmax reference maximum (exact here, a 16-bit deferred one there), so the fused error -- max-abs and relative rms --
must stay within 1.5 x the three-launch error; 1.5 covers the sampling spread of a maximum over ~10^5 outputs."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
C, H, D = 320, 8, 40
SHAPES = [(2, 128, 2), (4, 256, 2), (3, 128, 3)]          # (B, N, text rows): one / two workgroups per image, kv_bdiv 1 / 2 / 1
EPS = 1e-5


def make_case(B, N, Bt, L, dt, spike=False, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 17 * L + B + N)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(B, N, C) * (0.5 + 2.0 * torch.rand(B, N, 1, generator=g)) + 2.0 * r(B, N, 1)      # per-row scale and offset: LayerNorm matters
    wq = r(C, C) * C ** -0.5                                 # q ~ N(0, 1) per dim -> logits q.k / sqrt(40) of order 1
    bq = 0.1 * r(C)
    k, v = r(Bt, H, L, D), r(Bt, H, L, D)
    if spike:                                                # one token of the LAST key block whose logits reach about +15 (std 4, max over rows)
        k[:, :, L - 1] *= 4.0
    wo, bo = r(C, C) * C ** -0.5, 0.1 * r(C)
    c = dict(x=x.to(dt), wq=wq.to(dt), bq=bq, k=k.to(dt), v=v.to(dt), wo=wo.to(dt), bo=bo)
    return {n: t.cuda().contiguous() for n, t in c.items()}


def reference64(c, B, N, Bt):
    f = lambda t: t.double()
    x = f(c["x"])
    n = torch.nn.functional.layer_norm(x, (C,), None, None, EPS)
    q = (n @ f(c["wq"]).t() + f(c["bq"])).view(B, N, H, D).transpose(1, 2)                  # [B, H, N, D]
    rep = B // Bt
    k, v = f(c["k"]).repeat_interleave(rep, 0), f(c["v"]).repeat_interleave(rep, 0)
    att = torch.softmax(q @ k.transpose(2, 3) * D ** -0.5, dim=-1) @ v
    return x + att.transpose(1, 2).reshape(B, N, C) @ f(c["wo"]).t() + f(c["bo"])


def operands(c, L, dt):
    """K [Bt, H, L, 48] (pad column 1) and V^T [Bt, H, 64, LP] as the processors cache them per conditioning."""
    from imagdressing_amd import ops
    Bt = c["k"].shape[0]
    kb = ops.k_buffer((Bt, H, L, 48), D, dt, c["k"].device)
    kb[..., :D] = c["k"]
    LP = ops.pad64(L)
    vt = torch.zeros(Bt, H, 64, LP, dtype=dt, device=c["k"].device)
    vt[:, :, :D, :L] = c["v"].transpose(2, 3)
    return kb, vt, L, LP


def run(c, kv, B, Bt, fused, monkeypatch, residual=None, **kw):
    from imagdressing_amd import ops
    from imagdressing_amd.adapter import attention_processor as A
    monkeypatch.setattr(ops, "FUSED_XATTN", fused)
    x = c["x"]
    return A._fused_attention(x, H, wq_or_qkv=None, self_attn=False, kv1=kv, kv1_bdiv=B // Bt, wo=c["wo"], bo=c["bo"],
                              residual=x if residual is None else residual, q_ln=(c["wq"], c["bq"], EPS), **kw)


def errors(got, ref):
    d = got.double() - ref
    return float(d.abs().max()), float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def check_against_parent(fused, parent, ref, what):
    (fa, fr), (pa, pr) = errors(fused, ref), errors(parent, ref)
    print(f"{what}: fused max-abs {fa:.4e} rel-rms {fr:.4e} | three launches max-abs {pa:.4e} rel-rms {pr:.4e}")
    assert torch.isfinite(fused).all()
    assert fa <= 1.5 * pa and fr <= 1.5 * pr, (what, fa, pa, fr, pr)


@DT
@pytest.mark.parametrize("L", [77, 33, 96])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@torch.no_grad()
def test_fused_launch_is_as_accurate_as_three_launches(shape, L, dt, monkeypatch):
    B, N, Bt = shape
    c = make_case(B, N, Bt, L, dt)
    kv = operands(c, L, dt)
    ref = reference64(c, B, N, Bt)
    parent = run(c, kv, B, Bt, False, monkeypatch)
    fused = run(c, kv, B, Bt, True, monkeypatch)
    assert fused.dtype == dt and fused.shape == c["x"].shape
    check_against_parent(fused, parent, ref, f"B={B} N={N} Bt={Bt} L={L} {dt}")
    again = run(c, kv, B, Bt, True, monkeypatch)             # hits the cached K / V image and weight pack
    assert torch.equal(fused, again)
    assert torch.equal(again, run(c, kv, B, Bt, True, monkeypatch))


@DT
@pytest.mark.parametrize("L", [77, 33, 96])
@torch.no_grad()
def test_exact_maximum_in_the_last_key_block(L, dt, monkeypatch):
    B, N, Bt = 4, 256, 2
    c = make_case(B, N, Bt, L, dt, spike=True, seed=1)
    kv = operands(c, L, dt)
    ref = reference64(c, B, N, Bt)
    q = (torch.nn.functional.layer_norm(c["x"].double(), (C,), None, None, EPS) @ c["wq"].double().t() + c["bq"].double()).view(B, N, H, D)
    top = float((q.transpose(1, 2) @ c["k"].double().repeat_interleave(B // Bt, 0)[:, :, L - 1:].transpose(2, 3)).max() * D ** -0.5)
    assert 11.0 < top < 22.0, top                            # the spike token's logits reach about +15
    check_against_parent(run(c, kv, B, Bt, True, monkeypatch), run(c, kv, B, Bt, False, monkeypatch), ref, f"spike L={L} {dt} (top logit {top:.1f})")


def engine_attention(dt, kd=768, seed=3):
    from imagdressing_amd import unet
    from imagdressing_amd.adapter import attention_processor as A
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"a.to_q.weight": r(C, C) * C ** -0.5, "a.to_k.weight": r(C, kd) * kd ** -0.5, "a.to_v.weight": r(C, kd) * kd ** -0.5,
          "a.to_out.0.weight": r(C, C) * C ** -0.5, "a.to_out.0.bias": 0.1 * r(C)}
    attn = unet.Attention(sd, "a", H, torch.device("cuda"), dt)
    attn.set_processor(A.CAttnProcessor2_0("blk.attn2.processor", C, kd))
    norm = SimpleNamespace(weight=(1 + 0.3 * r(C)).cuda(), bias=(0.2 * r(C)).cuda())
    return attn, norm, g


@DT
@torch.no_grad()
def test_engine_attention_switch_on_and_off(dt, monkeypatch):
    """unet.Attention.__call__ with CAttnProcessor2_0, layernorm= and residual=: the switch changes the launch count, not the result."""
    from imagdressing_amd import ops
    from imagdressing_amd.adapter import attention_processor as A
    attn, norm, g = engine_attention(dt)
    B, N, L = 4, 256, 77
    h = (torch.randn(B, N, C, generator=g) * 1.5 + torch.randn(B, N, 1, generator=g)).to(dt).cuda()
    ehs = torch.randn(2, L, 768, generator=g).to(dt).cuda()
    calls = []
    real = ops.text_xattn
    monkeypatch.setattr(ops, "text_xattn", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops, "FUSED_XATTN", False)
    off = attn(h, encoder_hidden_states=ehs, residual=h, layernorm=(norm, EPS))
    assert not calls
    monkeypatch.setattr(ops, "FUSED_XATTN", True)
    on = attn(h, encoder_hidden_states=ehs, residual=h, layernorm=(norm, EPS))
    assert len(calls) == 1 and on.shape == off.shape and on.dtype == dt
    # fp64 reference on the 16-bit operands both paths use: folded W_q' / b_q', the projected text K / V, W_o
    wq, bq = A._ln_folded_q(attn, norm.weight, norm.bias, dt, h.device)
    k, vt, _, _ = A._project_kv(ehs, A._layer_weights(attn, "kv", dt, h.device), H)
    c = dict(x=h, wq=wq, bq=bq, k=k[..., :D], v=vt[:, :, :D, :L].transpose(2, 3), wo=attn.to_out[0].weight, bo=attn.to_out[0].bias)
    check_against_parent(on, off, reference64(c, B, N, 2), f"engine attention {dt}")


@DT
@torch.no_grad()
def test_fallbacks_are_bit_identical_to_switch_off(dt, monkeypatch):
    """Shapes and call forms outside the fused kernel's domain take the three-launch path whatever the switch says."""
    from imagdressing_amd import ops
    attn, norm, g = engine_attention(dt, seed=5)

    def both(fn):
        monkeypatch.setattr(ops, "FUSED_XATTN", False)
        off = fn()
        monkeypatch.setattr(ops, "FUSED_XATTN", True)
        monkeypatch.setattr(ops, "text_xattn", lambda *a, **k: pytest.fail("the fused launch must not take this call"))
        on = fn()
        monkeypatch.undo()
        assert torch.equal(on, off)

    mk = lambda *s: torch.randn(*s, generator=g).to(dt).cuda()
    h192, h128, other = mk(2, 192, C), mk(2, 128, C), mk(2, 128, C)
    e77, e100 = mk(2, 77, 768), mk(2, 100, 768)
    both(lambda: attn(h192, encoder_hidden_states=e77, residual=h192, layernorm=(norm, EPS)))        # N % 128 != 0
    both(lambda: attn(h128, encoder_hidden_states=e100, residual=h128, layernorm=(norm, EPS)))       # L > 96
    both(lambda: attn(h128, encoder_hidden_states=e77, residual=other, layernorm=(norm, EPS)))       # a residual that is not x
    both(lambda: attn(h128, encoder_hidden_states=e77, residual=None, layernorm=(norm, EPS)))        # no residual
    c = make_case(2, 128, 2, 77, dt)
    kv = operands(c, 77, dt)
    s2 = torch.ones(2, device="cuda")
    both(lambda: run(c, kv, 2, 2, ops.FUSED_XATTN, monkeypatch, kv2=kv, kv2_bdiv=1, scale2=s2))       # a second key set
