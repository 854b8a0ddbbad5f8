"""Request-batched call vs solo calls: R distinct try-on requests (garment, prompt, latent, guidance scale) at 512 x 640 and 50 DDIM steps,
timed as ONE pipeline call and as R single-request calls on the same pipeline, in fp16 and bf16.  Prints one JSON line.

    python tools/multi_request_bench.py [--requests 4] [--reps 3] [--steps 50] [--no-decode]

Each form is timed eagerly and with the HIP-graph step replay (``enable_step_graph``); the summary compares the faster form of each.  The
garment UNet runs once per call in both forms (R garments at batch R in the batched call, one per solo call), and the VAE decode of the final
latents is inside the timed region unless --no-decode (the bench.py definition of an image)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def requests(R, width, height, device, dtype):
    gen = torch.Generator().manual_seed(2024)
    lh, lw = height // 8, width // 8
    guid = [5.0, 6.5, 7.5, 9.0, 6.0, 8.0, 5.5, 7.0][:R] if R <= 8 else [7.5] * R
    return [dict(prompt_embeds=(torch.randn(1, 77, 768, generator=gen) * 0.5).to(device),
                 negative_prompt_embeds=(torch.randn(1, 77, 768, generator=gen) * 0.5).to(device),
                 ref_clip_hidden_states=(torch.randn(1, 257, 1280, generator=gen) * 0.5).to(device=device, dtype=dtype),
                 ref_image_latents=torch.randn(1, 4, lh, lw, generator=gen).to(device),
                 latents=torch.randn(1, 4, lh, lw, generator=gen).to(device), guidance_scale=guid[r]) for r in range(R)]


def batched(reqs):
    kw = {k: torch.cat([q[k] for q in reqs]) for k in ("prompt_embeds", "negative_prompt_embeds", "ref_clip_hidden_states",
                                                        "ref_image_latents", "latents")}
    kw["guidance_scale"] = [q["guidance_scale"] for q in reqs]
    return kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=4)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-decode", dest="decode", action="store_false", default=True)
    args = ap.parse_args()
    import bench
    from imagdressing_amd import ops
    dev = torch.device("cuda", 0)
    R = args.requests
    result = dict(tool="multi_request_bench", requests=R, width=args.width, height=args.height, ddim_steps=args.steps, reps=args.reps,
                  decode=args.decode, device=torch.cuda.get_device_name(dev))
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        pipe = bench.build_pipeline(dev, dtype, 0)
        if args.decode:
            from imagdressing_amd.vae import AutoencoderKL
            pipe.vae = AutoencoderKL.random_init(seed=5, device=dev, dtype=dtype)
        reqs = requests(R, args.width, args.height, dev, dtype)
        common = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
                      num_inference_steps=args.steps, num_images_per_prompt=1, output_type="pt" if args.decode else "latent")

        def run_batched():
            return pipe(**common, **batched(reqs)).images

        def run_solo():
            return torch.cat([pipe(**common, **q).images for q in reqs])

        res = {}
        outs = {}
        for form, fn in (("batched", run_batched), ("solo", run_solo)):
            for graph in (False, True):
                pipe.enable_step_graph(graph)
                outs[(form, graph)] = fn()                     # warm-up (kernel selection, caches, graph capture paths)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    out = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.reps
                res[f"{form}_{'graph' if graph else 'eager'}_s_per_call"] = round(dt, 4)
                res[f"{form}_{'graph' if graph else 'eager'}_finite"] = bool(torch.isfinite(out).all().item())
        pipe.enable_step_graph(False)
        best_b = min(res["batched_eager_s_per_call"], res["batched_graph_s_per_call"])
        best_s = min(res["solo_eager_s_per_call"], res["solo_graph_s_per_call"])
        d = (outs[("batched", False)].float() - outs[("solo", False)].float())
        res.update(batched_images_per_s=round(R / best_b, 3), solo_images_per_s=round(R / best_s, 3),
                   batched_ms_per_image=round(1000 * best_b / R, 1), solo_ms_per_image=round(1000 * best_s / R, 1),
                   speedup=round(best_s / best_b, 3),
                   batched_vs_solo_rel_rms=float(d.pow(2).mean().sqrt() / outs[("solo", False)].float().pow(2).mean().sqrt()))
        result[name] = res
        del pipe, outs
        ops.clear_workspaces()
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
