"""ops.pack_text_xattn / ops.pack_text_kv (operands of the one-launch text cross-attention, csrc/row_xattn.hip) are an exact
re-parametrisation: a float64 emulation of what the kernel READS -- every operand fetched through the kernel's own LDS address
arithmetic (piece swizzle of the weight chunks, head padding to 48 rows, rotated K rows, accumulator-ordered V^T columns, the
all-ones row, the mask column) and combined in the kernel's register order -- reproduces

    out = x + b_o + W_o concat_h softmax(q_h K_h^T / sqrt(d)) V_h,     q = LN(x; gamma, beta) W_q^T

on the original parameters.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as F

C, H, D, DP, LMAX = 320, 8, 40, 48, 96
CHUNK = 64 * 320                 # elements of an LDS ring slot
KROW, VROW = 48, 104             # elements per K / V^T image row
HEADB = LMAX * KROW + DP * VROW  # 9600


def acc_row(r, hi):              # row of a 32 x 32 MFMA accumulator block held by register r of lane half hi
    return (r & 3) + 8 * (r >> 2) + 4 * hi


def weight_chunk_as_read(chunk):
    """[64 rows, 320 k] as the fragment reads of a weight chunk see it: lane (row, hi), step s reads the 16-byte piece at position
    (2 s) ^ (hi ^ ((row >> 1) & 7)) of LDS row `row`; its 8 elements are contraction slots 16 s + 8 hi .. + 7."""
    flat = chunk.reshape(-1)
    a = torch.empty(64, C, dtype=flat.dtype)
    for row in range(64):
        for s in range(20):
            for hi in range(2):
                pos = (2 * s) ^ (hi ^ ((row >> 1) & 7))
                a[row, 16 * s + 8 * hi:16 * s + 8 * hi + 8] = flat[row * C + pos * 8:row * C + pos * 8 + 8]
    return a


def emulate(x, pk, img, kv_bdiv, rows_per_image, q_scale, eps=1e-5):
    M = x.shape[0]
    n = F.layer_norm(x, (C,), None, None, eps)              # the kernel normalises WITHOUT affine
    w, bq, bo = pk["w"], pk["bq"].double(), pk["bo"].double()
    out = torch.empty(M, C, dtype=x.dtype)
    wa = [weight_chunk_as_read(w[64 * c:64 * c + 64]) for c in range(11)]
    for m0 in range(0, M, rows_per_image):                  # (one conditioning row per image)
        rows = slice(m0, m0 + rows_per_image)
        tb = (m0 // rows_per_image) // kv_bdiv
        o_groups = {}                                       # (global head, group j, hi) -> [rows, 4] : O registers of a lane half
        for chh in range(2):
            # stage 1: six 32-row blocks of this wave half; block rows leave as B fragments of 8 consecutive rows
            qw = torch.empty(rows_per_image, 192, dtype=x.dtype)
            for c in range(6):
                a = wa[c][32 * chh:32 * chh + 32]
                qw[:, 32 * c:32 * c + 32] = (n[rows] @ a.t() + bq[64 * c + 32 * chh:64 * c + 32 * chh + 32]) * q_scale
            for hl in range(4):
                q = qw[:, 48 * hl:48 * hl + 48].clone()     # fragments 3 hl .. 3 hl + 2
                q[:, 40] = 1.0                              # the pad slot
                slot = img[tb, hl].reshape(-1)
                base = chh * HEADB
                kmat = torch.empty(LMAX, DP, dtype=x.dtype)
                for key in range(LMAX):
                    col = key % 32
                    for t in range(3):
                        for hi in range(2):
                            pos = (2 * t + hi + 3 * ((col >> 3) & 1)) % 6
                            o = base + key * KROW + pos * 8
                            kmat[key, 16 * t + 8 * hi:16 * t + 8 * hi + 8] = slot[o:o + 8]
                s = q @ kmat.t()                            # [rows, 96]: S^T block kb, register r of half hi = key 32 kb + acc_row(r, hi)
                p = torch.exp2(s - s.max(dim=1, keepdim=True).values)
                vbase = base + LMAX * KROW
                oacc = torch.zeros(rows_per_image, DP, dtype=x.dtype)
                for kb in range(3):
                    for g in range(2):
                        for hi in range(2):
                            for e in range(8):
                                key = 32 * kb + acc_row(8 * g + e, hi)       # packed P register e of fragment (kb, g)
                                colv = (2 * (2 * kb + g) + hi) * 8 + e       # contraction slot -> V^T image column
                                vcol = slot[vbase + colv:vbase + DP * VROW:VROW]           # rows d = 0..47 at d * VROW + colv
                                oacc += p[:, key:key + 1] * vcol[None, :]
                o16 = oacc[:, :41] / oacc[:, 40:41]
                assert torch.all(o16[:, 40] == 1.0) and torch.all(oacc[:, 41:] == 0)
                for j in range(5):
                    for hi in range(2):
                        o_groups[(4 * chh + hl, j, hi)] = o16[:, 8 * j + 4 * hi:8 * j + 4 * hi + 4]
        # stage 3: B fragment s, lane half hi, slot e = register e % 4 of channel group 2 s + e // 4 (list order 5 h + j)
        bmat = torch.empty(rows_per_image, C, dtype=x.dtype)
        for s in range(20):
            for hi in range(2):
                for e in range(8):
                    G = 2 * s + e // 4
                    bmat[:, 16 * s + 8 * hi + e] = o_groups[(G // 5, G % 5, hi)][:, e % 4]
        for co in range(5):
            a = wa[6 + co]
            out[rows, 64 * co:64 * co + 64] = bmat @ a.t() + bo[64 * co:64 * co + 64] + x[rows, 64 * co:64 * co + 64]
    return out


@pytest.mark.parametrize("L", [77, 33, 96])
def test_packed_operands_reproduce_the_plain_formula(L):
    from imagdressing_amd import ops
    g = torch.Generator().manual_seed(L)
    f64 = torch.float64
    B, N, Bt = 2, 4, 2                                      # (the emulation does not need 128-row images)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).to(f64)      # fp32-representable: the packer keeps biases in fp32
    x = r(B * N, C) * 1.5 + r(B * N, 1)
    wq, wo, bo = r(C, C) * C ** -0.5, r(C, C) * C ** -0.5, r(C)
    gamma, beta = 1 + 0.3 * r(C), 0.2 * r(C)
    k, v = r(Bt, H, L, D), r(Bt, H, L, D)
    # the operands the three-launch path caches per conditioning: K [Bt, H, L, 48] with pad column 1, V^T [Bt, H, 64, LP]
    kbuf = torch.zeros(Bt, H, L, DP, dtype=f64); kbuf[..., :D] = k; kbuf[..., D] = 1.0
    LP = ops.pad64(L)
    vt = torch.zeros(Bt, H, 64, LP, dtype=f64); vt[:, :, :D, :L] = v.transpose(2, 3)
    bq = (wq @ beta).float()                                # fold_layernorm_affine: W' = W diag(gamma), b' = W beta (fp32)
    pk = ops._pack_text_xattn(wq * gamma[None, :], bq, wo, bo.float())
    img = ops._pack_text_kv(kbuf, vt, L)
    assert pk["w"].shape == (11 * 64, C) and pk["bq"].shape == (6 * 64,) and img.shape == (Bt, 4, CHUNK)
    q_scale = D ** -0.5 * math.log2(math.e)
    got = emulate(x, pk, img, kv_bdiv=B // Bt, rows_per_image=N, q_scale=q_scale)
    q = (F.layer_norm(x, (C,), gamma, None, 1e-5) @ wq.t() + bq.double()).view(B, N, H, D).transpose(1, 2)      # beta enters through b'
    att = torch.softmax(q @ k.transpose(2, 3) * D ** -0.5, dim=-1) @ v                                          # [B, H, N, D] (Bt == B)
    ref = x + att.transpose(1, 2).reshape(B * N, C) @ wo.t() + bo
    assert torch.allclose(got, ref, atol=1e-9, rtol=1e-9), float((got - ref).abs().max())


def test_parameter_block_mirrors_the_header_and_is_size_checked():
    """imd_xattn_params: the ctypes mirror follows the header field for field, a foreign struct_bytes is refused before any field
    is read, and the geometry predicate answers without a GPU."""
    import ctypes
    import os
    import re
    from imagdressing_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "imagdressing_hip.h")).read()
    body = re.search(r"typedef struct imd_xattn_params \{(.*?)\} imd_xattn_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert [f[0] for f in _lib.XattnParams._fields_] == fields
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    p = _lib.XattnParams()
    assert p.struct_bytes == ctypes.sizeof(_lib.XattnParams)
    p.M, p.C, p.heads, p.L, p.rows_per_image, p.kv_bdiv, p.text_rows, p.x_ld, p.out_ld = 8 * 4096, 320, 8, 77, 4096, 4, 2, 320, 320
    assert lib.imd_text_xattn320_supported(ctypes.byref(p)) == 1
    for field, bad in (("L", 97), ("L", 0), ("rows_per_image", 192), ("heads", 5), ("C", 640), ("text_rows", 3), ("x_ld", 324), ("dtype", 2)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert lib.imd_text_xattn320_supported(ctypes.byref(p)) == 0, field
        setattr(p, field, keep)
    p.struct_bytes -= 8
    assert lib.imd_text_xattn320_supported(ctypes.byref(p)) == 0
    assert lib.imd_text_xattn320(ctypes.byref(p), None) != 0 and b"parameter block is" in lib.imd_last_error()


def test_cached_packs_are_reused_and_dropped():
    from imagdressing_amd import ops
    k = torch.zeros(1, H, 5, DP); vt = torch.zeros(1, H, 64, 64)
    a = ops.pack_text_kv(k, vt, 5)
    assert ops.pack_text_kv(k, vt, 5) is a
    w = torch.zeros(C, C); b = torch.zeros(C)
    p = ops.pack_text_xattn(w, b, w, None)
    assert ops.pack_text_xattn(w, b, w, None) is p
    w.add_(1.0)                                             # an in-place edit is seen
    assert ops.pack_text_xattn(w, b, w, None) is not p
    ops.clear_workspaces()
    assert ops.pack_text_kv(k, vt, 5) is not a
    with pytest.raises(Exception):
        ops.pack_text_kv(k, vt, 97)
