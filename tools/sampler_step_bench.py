"""Per-step cost of the samplers on one box: DDIM (``imd_ddim_cfg_step``, the path every earlier commit runs), DPM-Solver++, Euler and PNDM
(``imd_sampler_step``) and UniPC (three ``imd_lincomb`` launches + one), at the geometry of BASELINE configs[1] (512 x 640, one image), and
images/s of DDIM-50 against DPM-Solver++-20.  Prints one JSON line and, with --out, writes it to a file (profiles/sampler_step_bench.json).

    python tools/sampler_step_bench.py [--steps 20] [--reps 5] [--dtype fp16] [--out profiles/sampler_step_bench.json]

The repeats are INTERLEAVED (one run of every sampler per round, the order rotating) so that clock and thermal drift lands on all of them
alike; each sampler is timed eagerly and under ``enable_step_graph`` where it applies.  Per-step time = time of a pipeline call to latents
(garment UNet included, no VAE decode) / UNet calls of that call (PNDM makes steps + 1).  The expectation this tool confirms or refutes: a
sampler on the fused step costs what DDIM costs per step, inside DDIM's own run-to-run spread -- one elementwise launch among ~500."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def schedulers():
    from imagdressing_amd import scheduler as S
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    return {"ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kw),
            "dpmpp_2m": lambda: S.DPMSolverMultistepScheduler(**kw),
            "euler": lambda: S.EulerDiscreteScheduler(**kw),
            "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **kw),
            "unipc": lambda: S.UniPCMultistepScheduler(**kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda", 0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    pipe = bench.build_pipeline(dev, dtype, 0)
    gen = torch.Generator().manual_seed(2024)
    lh, lw = args.height // 8, args.width // 8
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
              num_images_per_prompt=1, guidance_scale=7.5, output_type="latent",
              prompt_embeds=(torch.randn(1, 77, 768, generator=gen) * 0.5).to(dev),
              negative_prompt_embeds=(torch.randn(1, 77, 768, generator=gen) * 0.5).to(dev),
              ref_clip_hidden_states=(torch.randn(1, 257, 1280, generator=gen) * 0.5).to(device=dev, dtype=dtype),
              ref_image_latents=torch.randn(1, 4, lh, lw, generator=gen).to(dev), latents=torch.randn(1, 4, lh, lw, generator=gen).to(dev))
    mk = schedulers()
    runs = [(name, graph, args.steps) for name in mk for graph in (False, True) if not (graph and name == "unipc")]
    runs += [("ddim", True, 50), ("dpmpp_2m", True, 20)]          # the images/s comparison (20 appears twice when --steps 20: fine)
    runs = list(dict.fromkeys(runs))

    def call(name, graph, steps):
        pipe.scheduler = mk[name]()
        pipe.enable_step_graph(graph)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(num_inference_steps=steps, **kw).images
        torch.cuda.synchronize()
        return time.perf_counter() - t0, bool(torch.isfinite(out).all().item())
    times = {r: [] for r in runs}
    finite = {}
    for r in runs:                                                   # warm-up: kernel selection, caches, graph capture
        finite[r] = call(*r)[1]
    for rep in range(args.reps):
        for r in runs[rep % len(runs):] + runs[:rep % len(runs)]:
            times[r].append(call(*r)[0])
    pipe.enable_step_graph(False)
    res = dict(tool="sampler_step_bench", width=args.width, height=args.height, dtype=args.dtype, reps=args.reps,
               device=torch.cuda.get_device_name(dev), samplers={})
    for (name, graph, steps), ts in times.items():
        calls = steps + 1 if name == "pndm" else steps
        res["samplers"][f"{name}_{steps}_{'graph' if graph else 'eager'}"] = dict(
            unet_calls=calls, ms_per_call_median=round(1e3 * statistics.median(ts), 2), ms_per_call_min=round(1e3 * min(ts), 2),
            ms_per_call_max=round(1e3 * max(ts), 2), ms_per_step_median=round(1e3 * statistics.median(ts) / calls, 3),
            ms_per_step_min=round(1e3 * min(ts) / calls, 3), ms_per_step_max=round(1e3 * max(ts) / calls, 3), finite=finite[(name, graph, steps)])
    s = res["samplers"]
    res["images_per_s"] = {"ddim_50": round(1.0 / (s["ddim_50_graph"]["ms_per_call_median"] / 1e3), 3),
                           "dpmpp_2m_20": round(1.0 / (s["dpmpp_2m_20_graph"]["ms_per_call_median"] / 1e3), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
