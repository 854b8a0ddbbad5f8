"""Per-request ControlNet scale and guidance window in one batch (``enable_request_control_scales``): what the rows route costs.

    python tools/control_rows_bench.py [--requests 4] [--reps 5] [--steps 20] [--dtypes fp16,bf16] [--out profiles/control_rows_bench.json]

One MI355X, one process, fp16 and bf16, 512 x 640, DPM-Solver++-20, full-width random-init SD1.5 weights; every figure is the median
[min - max] over ``reps`` repeats with the arms INTERLEAVED (a, b, c, a, b, c, ...) after one warm-up of each.  No speed-up is claimed.

1. The kernel alone (``imd_residual_scale_rows``): the 13 residuals of R requests (2 R batch rows), every row at a scale other than 1 --
   us per launch (HIP events around ``iters`` back-to-back launches), bytes moved (read + written), TB/s -- and the same with every row at 1.0.
2. The ControlNet pipeline, R distinct requests (garment, prompt, pose, latent, guidance):
     (a) one call of R requests with R different (scale, start, end) triples -- the rows route
     (b) the same R as R solo folded calls
     (c) one call of R with equal values -- the folded route of a batch
   (a)/(b), (a)/(c), and ``expected_a`` = (c) + steps x the kernel time.  ``library_calls``: the calls per entry point of one pipeline call
   (a counting proxy, in a run of its own): the switch off, and the switch on with equal values, must equal (c); (a) adds ``steps`` calls of
   imd_residual_scale_rows and nothing else.
3. The rows route under ``enable_step_graph`` against eager, for the record."""
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

TRIPLES = [(1.0, 0.0, 1.0), (0.5, 0.2, 1.0), (0.8, 0.0, 0.5), (1.3, 0.1, 0.9), (0.6, 0.0, 1.0), (0.9, 0.3, 0.7), (0.7, 0.0, 0.8), (0.4, 0.2, 0.6)]
WIDTHS = (320, 640, 1280, 1280)


def spread(xs, digits=4):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), n=len(xs))


def residual_shapes(h, w):
    """[h, w, channels] of the 13 ControlNet residuals of an h x w latent (SD1.5: conv_in, two per level, a downsample between levels, mid)"""
    out = [(h, w, WIDTHS[0])]
    for lv, c in enumerate(WIDTHS):
        out += [(h, w, c)] * 2
        if lv < len(WIDTHS) - 1:
            h, w = (h + 1) // 2, (w + 1) // 2
            out.append((h, w, c))
    return out + [(h, w, WIDTHS[-1])]


def kernel_alone(dtype, rows, h, w, iters, reps):
    from imagdressing_amd import ops
    segs = [(torch.randn(rows, *s, device="cuda") * 0.5).to(dtype) for s in residual_shapes(h, w)]
    per_row = sum(t[0].numel() for t in segs) * 2
    arms = {"all_rows_scaled": torch.full((rows,), 0.999, device="cuda"), "all_rows_one": torch.ones(rows, device="cuda")}
    us = {a: [] for a in arms}
    for s in arms.values():
        for _ in range(5):
            ops.residual_scale_rows(segs, s)
    for rep in range(reps):
        for a in (list(arms) if rep % 2 == 0 else list(arms)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                ops.residual_scale_rows(segs, arms[a])          # (0.999: the data neither grows nor dies over the launches)
            e1.record()
            torch.cuda.synchronize()
            us[a].append(e0.elapsed_time(e1) * 1e3 / iters)
    moved = 2 * per_row * rows
    med = statistics.median(us["all_rows_scaled"])
    return dict(rows=rows, segments=len(segs), bytes_per_row=per_row, bytes_moved=moved, us_per_launch={a: spread(v, 2) for a, v in us.items()},
                tb_per_s=round(moved / med / 1e6, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=4)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_rows_bench.json"))
    args = ap.parse_args()
    import bench
    from guidance_rescale_bench import CountingLib
    from imagdressing_amd import _lib, ops
    from imagdressing_amd import scheduler as S
    from imagdressing_amd import unet as E
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    dev = torch.device("cuda", 0)
    R, W, H = args.requests, args.width, args.height
    tr = TRIPLES[:R]
    res = dict(tool="control_rows_bench", device=torch.cuda.get_device_name(dev), requests=R, width=W, height=H, sampler="DPM-Solver++",
               steps=args.steps, reps=args.reps, triples=tr, note="synthetic weights: the figures say nothing about image quality", results={})
    for dname in args.dtypes.split(","):
        dt = torch.float16 if dname == "fp16" else torch.bfloat16
        kern = kernel_alone(dt, 2 * R, H // 8, W // 8, args.iters, args.reps)
        base = bench.build_pipeline(dev, dt, 0)
        pipe = IMAGDressing_v1(vae=None, reference_unet=base.reference_unet, unet=base.unet, tokenizer=None, text_encoder=None,
                               controlnet=E.ControlNetModel.random_init(seed=9, device=dev, dtype=dt), image_encoder=None, ImgProj=base.ImgProj,
                               scheduler=S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                                       beta_schedule="scaled_linear"))
        g = torch.Generator().manual_seed(77)
        rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale        # noqa: E731
        reqs = [dict(prompt_embeds=rn(1, 77, 768, scale=0.5).to(dev), negative_prompt_embeds=rn(1, 77, 768, scale=0.5).to(dev),
                     ref_clip_hidden_states=rn(1, 257, 1280, scale=0.5).to(device=dev, dtype=dt), ref_image_latents=rn(1, 4, H // 8, W // 8).to(dev),
                     latents=rn(1, 4, H // 8, W // 8).to(dev), pose_image=torch.rand(1, 3, H, W, generator=g).to(dev)) for _ in range(R)]
        guidance = [5.0, 6.5, 7.5, 9.0, 6.0, 8.0, 5.5, 7.0][:R]
        common = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=W, height=H, num_inference_steps=args.steps,
                      num_images_per_prompt=1, output_type="latent")
        batched = {k: torch.cat([q[k] for q in reqs]) for k in reqs[0]}
        mixed = dict(controlnet_conditioning_scale=[t[0] for t in tr], control_guidance_start=[t[1] for t in tr], control_guidance_end=[t[2] for t in tr])
        equal = dict(controlnet_conditioning_scale=tr[1][0], control_guidance_start=0.0, control_guidance_end=1.0)

        def arm_a():
            pipe.enable_request_control_scales()
            return pipe(**common, **batched, guidance_scale=guidance, **mixed).images

        def arm_b():
            pipe.disable_request_control_scales()
            return torch.cat([pipe(**common, **q, guidance_scale=guidance[r], controlnet_conditioning_scale=tr[r][0], control_guidance_start=tr[r][1],
                                   control_guidance_end=tr[r][2]).images for r, q in enumerate(reqs)])

        def arm_c():
            pipe.disable_request_control_scales()
            return pipe(**common, **batched, guidance_scale=guidance, **equal).images

        def arm_on_equal():
            pipe.enable_request_control_scales()
            return pipe(**common, **batched, guidance_scale=guidance, **dict(equal, controlnet_conditioning_scale=[tr[1][0]] * R)).images

        def graphed(fn):
            def run():
                pipe.enable_step_graph(True)
                try:
                    return fn()
                finally:
                    pipe.enable_step_graph(False)
            return run

        arms = (("a_mixed_rows", arm_a), ("b_solo_folded", arm_b), ("c_equal_folded", arm_c), ("a_mixed_rows_step_graph", graphed(arm_a)))
        outs, times = {}, {n: [] for n, _ in arms}
        for n, fn in arms:          # warm-up: kernel selection, workspaces
            outs[n] = fn()
        torch.cuda.synchronize()
        # library calls per entry point: one counted call of each arm, not timed
        real, counts = _lib.load(), {}
        for n, fn in (("a_mixed_rows", arm_a), ("c_equal_folded", arm_c), ("on_equal", arm_on_equal)):
            _lib._lib = proxy = CountingLib(real)
            try:
                outs["counted " + n] = fn()
            finally:
                _lib._lib = real
            counts[n] = dict(proxy.counts)
        for rep in range(args.reps):
            for n, fn in (arms if rep % 2 == 0 else arms[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[n] = fn()
                torch.cuda.synchronize()
                times[n].append(time.perf_counter() - t0)
        pipe.disable_request_control_scales()
        med = {n: statistics.median(v) for n, v in times.items()}
        kern_s = kern["us_per_launch"]["all_rows_scaled"]["median"] * 1e-6
        d = outs["a_mixed_rows"].float() - outs["b_solo_folded"].float()
        res["results"][dname] = dict(
            kernel=kern, seconds_per_arm={n: spread(v) for n, v in times.items()},
            ms_per_step={n: round(m / args.steps * 1e3, 3) for n, m in med.items()},
            a_over_b=round(med["a_mixed_rows"] / med["b_solo_folded"], 3), a_over_c=round(med["a_mixed_rows"] / med["c_equal_folded"], 3),
            expected_a_seconds=round(med["c_equal_folded"] + args.steps * kern_s, 4),
            graph_over_eager=round(med["a_mixed_rows_step_graph"] / med["a_mixed_rows"], 3),
            graph_bit_identical_to_eager=bool(torch.equal(outs["a_mixed_rows_step_graph"], outs["a_mixed_rows"])),
            library_calls_a_beyond_c={k: v - counts["c_equal_folded"].get(k, 0) for k, v in counts["a_mixed_rows"].items()
                                      if v != counts["c_equal_folded"].get(k, 0)},
            on_equal_same_calls_as_c=bool(counts["on_equal"] == counts["c_equal_folded"]),
            on_equal_bit_identical_to_c=bool(torch.equal(outs["counted on_equal"], outs["c_equal_folded"])),
            mixed_vs_solo_rel_rms=float(d.pow(2).mean().sqrt() / outs["b_solo_folded"].float().pow(2).mean().sqrt()),
            finite=bool(all(torch.isfinite(o).all().item() for o in outs.values())))
        del pipe, base
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
