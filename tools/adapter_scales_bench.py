"""Per-request face / LoRA scales in one batch (``enable_request_adapter_scales``): what the unfolded LoRA route costs in situ.

    python tools/adapter_scales_bench.py [--requests 4] [--reps 5] [--steps 20] [--dtype fp16] [--out profiles/adapter_scales_bench.json]

IP-Adapter + ControlNet pipeline (BASELINE configs[2] weights: rank-128 LoRA on every attention layer, 4 face tokens) at 512 x 640,
DPM-Solver++, R distinct requests (garment, prompt, pose, face, latent, guidance).  Three arms, ONE process, ``reps`` interleaved repeats
(a, b, c, a, b, c, ...) after one warm-up of each; median [min - max] seconds per arm:

  (a) one call, R different (ipa_scale, s_lora_scale, c_lora_scale) triples, switch on -- the unfolded route: one ``imd_lora_expand_rows``
      launch in front of each LoRA projection, whose K grows by the rank
  (b) the same R requests as R solo calls (each with its own triple folded into the weights; the fold of a new scale is inside the timing,
      as it would be when serving)
  (c) one call of R with equal scales -- the folded route of a batch

and the new kernel alone at the three real widths (HIP events around 20 back-to-back launches, median of ``reps``).  Prints one JSON line and
writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

TRIPLES = [(0.9, 0.2, 0.2), (0.3, 0.8, 0.0), (0.6, 0.5, 0.4), (1.0, 0.0, 0.7), (0.5, 0.5, 0.5), (0.2, 0.9, 0.1), (0.8, 0.3, 0.6), (0.4, 0.6, 0.3)]
GUIDANCE = [5.0, 6.5, 7.5, 9.0, 6.0, 8.0, 5.5, 7.0]


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def kernel_times(dtype, reps, R):
    """us per ``imd_lora_expand_rows`` launch at the shapes of a 512 x 640 call of R requests (2 R rows of the CFG batch)"""
    from imagdressing_amd import ops
    out = {}
    for C, tokens in ((320, 64 * 80), (640, 32 * 40), (1280, 16 * 20)):
        for T in (384, 128):          # q / k / v of a self-attention; to_q of a cross-attention / to_out
            M = 2 * R * tokens
            x = torch.randn(M, C, device="cuda").to(dtype)
            d = (torch.randn(T, C, device="cuda") * C ** -0.5).to(dtype)
            s = torch.rand(2 * R, device="cuda")
            o = torch.empty(M, C + T, device="cuda", dtype=dtype)
            ops.lora_expand_rows(x, d, s, tokens, out=o)
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    ops.lora_expand_rows(x, d, s, tokens, out=o)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1000 / 20)
            bytes_moved = (M * C + M * (C + T) + T * C) * 2
            out[f"C{C}_T{T}_M{M}"] = dict(us=spread(us), gb_per_s=round(bytes_moved / statistics.median(us) / 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=4)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapter_scales_bench.json"))
    args = ap.parse_args()
    import configs
    from imagdressing_amd import ops
    from imagdressing_amd import scheduler as S
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    R, W, H = args.requests, args.width, args.height
    pipe, _ = configs.build(3, dev, dt, batch=1, steps=args.steps)
    pipe.scheduler = S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    g = torch.Generator().manual_seed(77)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale        # noqa: E731
    reqs = [dict(prompt_embeds=rn(1, 77, 768, scale=0.5).to(dev), negative_prompt_embeds=rn(1, 77, 768, scale=0.5).to(dev),
                 ref_clip_hidden_states=rn(1, 257, 1280, scale=0.5).to(device=dev, dtype=dt), ref_image_latents=rn(1, 4, H // 8, W // 8).to(dev),
                 latents=rn(1, 4, H // 8, W // 8).to(dev), pose_image=torch.rand(1, 3, H, W, generator=g).to(dev),
                 faceid_embeds=rn(1, 512).to(dev), face_clip_hidden_states=rn(1, 257, 1280, scale=0.5).to(device=dev, dtype=dt),
                 face_uncond_clip_hidden_states=rn(1, 257, 1280, scale=0.5).to(device=dev, dtype=dt)) for _ in range(R)]
    common = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=W, height=H, num_inference_steps=args.steps,
                  num_images_per_prompt=1, image_scale=0.9, output_type="latent")
    batched = {k: torch.cat([q[k] for q in reqs]) for k in reqs[0]}
    tr = TRIPLES[:R]

    def arm_a():
        pipe.enable_request_adapter_scales()
        return pipe(**common, **batched, guidance_scale=GUIDANCE[:R], ipa_scale=[t[0] for t in tr], s_lora_scale=[t[1] for t in tr],
                    c_lora_scale=[t[2] for t in tr]).images

    def arm_b():
        pipe.disable_request_adapter_scales()
        return torch.cat([pipe(**common, **q, guidance_scale=GUIDANCE[r], ipa_scale=tr[r][0], s_lora_scale=tr[r][1], c_lora_scale=tr[r][2]).images
                          for r, q in enumerate(reqs)])

    def arm_c():
        pipe.disable_request_adapter_scales()
        return pipe(**common, **batched, guidance_scale=GUIDANCE[:R], ipa_scale=tr[0][0], s_lora_scale=tr[0][1], c_lora_scale=tr[0][2]).images

    arms = (("a_mixed_rows", arm_a), ("b_solo_folded", arm_b), ("c_equal_folded", arm_c))
    outs, times = {}, {n: [] for n, _ in arms}
    for n, fn in arms:          # warm-up: kernel selection, weight folds / augmented weights, workspaces
        outs[n] = fn()
    torch.cuda.synchronize()
    launches0 = ops.LORA_ROWS_COUNTER["launches"]
    for _ in range(args.reps):
        for n, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[n].append(time.perf_counter() - t0)
            outs[n] = out
    expand_per_call = (ops.LORA_ROWS_COUNTER["launches"] - launches0) // args.reps
    d = outs["a_mixed_rows"].float() - outs["b_solo_folded"].float()
    med = {n: statistics.median(v) for n, v in times.items()}
    res = dict(tool="adapter_scales_bench", device=torch.cuda.get_device_name(dev), dtype=args.dtype, requests=R, width=W, height=H,
               sampler="DPM-Solver++", steps=args.steps, reps=args.reps, triples=tr,
               seconds_per_arm={n: spread(v) for n, v in times.items()},
               a_over_b=round(med["a_mixed_rows"] / med["b_solo_folded"], 3), a_over_c=round(med["a_mixed_rows"] / med["c_equal_folded"], 3),
               a_over_b_per_repeat=[round(x / y, 3) for x, y in zip(times["a_mixed_rows"], times["b_solo_folded"])],
               a_over_c_per_repeat=[round(x / y, 3) for x, y in zip(times["a_mixed_rows"], times["c_equal_folded"])],
               expand_launches_per_mixed_call=expand_per_call,
               mixed_vs_solo_rel_rms=float(d.pow(2).mean().sqrt() / outs["b_solo_folded"].float().pow(2).mean().sqrt()),
               finite=bool(all(torch.isfinite(o).all().item() for o in outs.values())),
               lora_expand_rows_kernel=kernel_times(dt, args.reps, R))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
