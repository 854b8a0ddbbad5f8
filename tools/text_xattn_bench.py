"""One-launch text cross-attention (row_xattn.hip) against the three launches it replaces (norm2 + to_q, attention over 77 text keys,
to_out + residual) at the 64x64 level (M = 8 x 4096 = 32768 rows, C = 320, 8 heads); activations rotate over 12 sets (252 MB: past
the 256 MB of Infinity Cache together with the outputs, so x comes from HBM as in the running loop).  Usage: text_xattn_bench.py [bf16|fp16]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from imagdressing_amd import ops
from imagdressing_amd.adapter import attention_processor as A

def timed(fn, iters=36):
    for _ in range(12): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 1)

dt = torch.bfloat16 if (len(sys.argv) < 2 or sys.argv[1] == "bf16") else torch.float16
B, N, Cc, H, D, L, Bt = 8, 4096, 320, 8, 40, int(os.environ.get("XA_L", 77)), 2
NS = 12
xs = [(torch.randn(B, N, Cc, device="cuda") * 1.5 + torch.randn(B, N, 1, device="cuda")).to(dt) for _ in range(NS)]
wq = (torch.randn(Cc, Cc, device="cuda") * Cc ** -0.5).to(dt); bq = torch.randn(Cc, device="cuda") * 0.1
wo = (torch.randn(Cc, Cc, device="cuda") * Cc ** -0.5).to(dt); bo = torch.randn(Cc, device="cuda") * 0.1
k = ops.k_buffer((Bt, H, L, 48), D, dt, torch.device("cuda")); k[..., :D] = torch.randn(Bt, H, L, D, device="cuda").to(dt)
LP = ops.pad64(L)
vt = torch.zeros(Bt, H, 64, LP, dtype=dt, device="cuda"); vt[:, :, :D, :L] = torch.randn(Bt, H, D, L, device="cuda").to(dt)
kv = (k, vt, L, LP)
i = [0]
def call(fused):
    def fn():
        j = i[0] % NS; i[0] += 1
        ops.FUSED_XATTN = fused
        A._fused_attention(xs[j], H, wq_or_qkv=None, self_attn=False, kv1=kv, kv1_bdiv=B // Bt, wo=wo, bo=bo, residual=xs[j], q_ln=(wq, bq, 1e-5))
    return fn
row = dict(M=B * N, L=L, dtype=str(dt))
for rep in range(2):
    row[f"three_launches_us_{rep}"] = timed(call(False)); row[f"fused_us_{rep}"] = timed(call(True))
M = B * N
fl = 2 * 2.0 * M * Cc * Cc + 4.0 * M * Cc * L          # the two projections + Q K^T and P V over the L keys
row["fused_tflops"] = round(fl / row["fused_us_1"] / 1e6, 1)
row["bound_us_42MB_at_5TBs"] = round(2 * M * Cc * 2 / 5e12 * 1e6, 1)
print(json.dumps(row), flush=True)
