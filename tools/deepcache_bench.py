"""What DeepCache (``pipe.enable_deepcache``) buys on one box: the base pipeline at 512 x 640, one image and four requests in one call,
DDIM-50 and DPM-Solver++-20, fp16 and bf16 -- the same tree with the switch off (eager, and under ``enable_step_graph``, which the
switch-on loop cannot use) and on with (cache_interval, depth) in {(2, 1), (3, 1), (3, 2), (5, 1)}.  Prints one JSON line and, with
--out, writes it to a file (profiles/deepcache_bench.json).

    python tools/deepcache_bench.py [--reps 5] [--out profiles/deepcache_bench.json]

The repeats are INTERLEAVED (one run of every arm per round, the order rotating) so that clock and thermal drift lands on all of them
alike.  ms per call = a pipeline call to latents (garment UNet included, no VAE decode), median [min - max] over the repeats.  ms per
full / shallow step: a second, instrumented call per arm and repeat that synchronises in a step callback and reads the wall clock -- the
median over every step of that kind (call 0 left out: it also fills the processors' K / V caches).  A synchronised step cannot overlap its
host work with the previous step's kernels, so these two add up to MORE than the un-instrumented call; they are there to compare a shallow
step with a full one.  ``rel_rms_vs_off`` is the distance of the final latents from the switch-off arm's: the weights are synthetic, so it
documents the mechanism (the cached loop really computes something else) and says NOTHING about image quality on a real checkpoint."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ARMS = [("off_eager", None), ("off_graph", None), ("on_2_1", (2, 1)), ("on_3_1", (3, 1)), ("on_3_2", (3, 2)), ("on_5_1", (5, 1))]
SAMPLERS = [("ddim_50", "ddim", 50), ("dpmpp_2m_20", "dpm", 20)]


def scheduler(name):
    from imagdressing_amd import scheduler as S
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    if name == "ddim":
        return S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kw)
    return S.DPMSolverMultistepScheduler(**kw)


def inputs(R, width, height, device, dtype):
    gen = torch.Generator().manual_seed(2024)
    lh, lw = height // 8, width // 8
    kw = dict(prompt_embeds=(torch.randn(R, 77, 768, generator=gen) * 0.5).to(device),
              negative_prompt_embeds=(torch.randn(R, 77, 768, generator=gen) * 0.5).to(device),
              ref_clip_hidden_states=(torch.randn(R, 257, 1280, generator=gen) * 0.5).to(device=device, dtype=dtype),
              ref_image_latents=torch.randn(R, 4, lh, lw, generator=gen).to(device), latents=torch.randn(R, 4, lh, lw, generator=gen).to(device))
    kw["guidance_scale"] = 7.5 if R == 1 else [5.0, 6.5, 7.5, 9.0, 6.0, 8.0, 5.5, 7.0][:R]
    return kw


def spread(ts, scale=1e3):
    return dict(median=round(scale * statistics.median(ts), 3), min=round(scale * min(ts), 3), max=round(scale * max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--requests", type=int, default=4)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from imagdressing_amd import ops
    from imagdressing_amd.dressing_sd.pipelines._base import deepcache_plan
    dev = torch.device("cuda", 0)
    res = dict(tool="deepcache_bench", width=args.width, height=args.height, reps=args.reps, device=torch.cuda.get_device_name(dev),
               note="synthetic weights: rel_rms_vs_off documents the mechanism and says nothing about image quality",
               arms={name: (None if cfg is None else dict(cache_interval=cfg[0], depth=cfg[1])) for name, cfg in ARMS}, results={})
    for dname in args.dtypes.split(","):
        dtype = torch.float16 if dname == "fp16" else torch.bfloat16
        pipe = bench.build_pipeline(dev, dtype, 0)
        for bname, R in (("one_image", 1), (f"{args.requests}_requests", args.requests)):
            kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
                      num_images_per_prompt=1, output_type="latent", **inputs(R, args.width, args.height, dev, dtype))
            for sname, sched, steps in SAMPLERS:

                def call(arm, cfg, callback=None):
                    pipe.scheduler = scheduler(sched)
                    pipe.enable_step_graph(arm == "off_graph")
                    if cfg is None:
                        pipe.disable_deepcache()
                    else:
                        pipe.enable_deepcache(cache_interval=cfg[0], depth=cfg[1])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = pipe(num_inference_steps=steps, callback=callback, **kw).images
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, out

                def per_step(arm, cfg):
                    """one call with a synchronising callback -> ([seconds of full steps], [seconds of shallow steps]), call 0 left out"""
                    marks = []

                    def cb(i, t, z):
                        torch.cuda.synchronize()
                        marks.append(time.perf_counter())
                    call(arm, cfg, cb)
                    plan = deepcache_plan(len(marks), 1 if cfg is None else cfg[0])
                    full = [marks[i] - marks[i - 1] for i in range(1, len(marks)) if plan[i]]
                    shallow = [marks[i] - marks[i - 1] for i in range(1, len(marks)) if not plan[i]]
                    return full, shallow

                outs, times, full_t, shallow_t = {}, {a: [] for a, _ in ARMS}, {a: [] for a, _ in ARMS}, {a: [] for a, _ in ARMS}
                for arm, cfg in ARMS:                                       # warm-up: kernel selection, caches, graph capture
                    outs[arm] = call(arm, cfg)[1].float()
                for rep in range(args.reps):
                    k = rep % len(ARMS)
                    for arm, cfg in ARMS[k:] + ARMS[:k]:
                        times[arm].append(call(arm, cfg)[0])
                        if arm != "off_graph":                              # (a callback makes that arm the eager one)
                            f, s = per_step(arm, cfg)
                            full_t[arm] += f
                            shallow_t[arm] += s
                off = outs["off_eager"]
                block = {}
                for arm, cfg in ARMS:
                    d = outs[arm] - off
                    e = dict(ms_per_call=spread(times[arm]), finite=bool(torch.isfinite(outs[arm]).all().item()),
                             rel_rms_vs_off=float(d.pow(2).mean().sqrt() / off.pow(2).mean().sqrt()),
                             speedup_vs_off_eager=round(statistics.median(times["off_eager"]) / statistics.median(times[arm]), 3),
                             speedup_vs_off_graph=round(statistics.median(times["off_graph"]) / statistics.median(times[arm]), 3))
                    if full_t[arm]:
                        e["ms_per_full_step"] = spread(full_t[arm])
                    if shallow_t[arm]:
                        e["ms_per_shallow_step"] = spread(shallow_t[arm])
                    if cfg is not None:
                        e["full_calls"] = sum(deepcache_plan(steps, cfg[0]))
                        e["shallow_calls"] = steps - e["full_calls"]
                    block[arm] = e
                res["results"].setdefault(dname, {}).setdefault(bname, {})[sname] = block
                print(f"# {dname} {bname} {sname}: " + ", ".join(f"{a} {block[a]['ms_per_call']['median']:.1f} ms" for a, _ in ARMS), file=sys.stderr, flush=True)
        pipe.enable_step_graph(False)
        pipe.disable_deepcache()
        del pipe
        ops.clear_workspaces()
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
