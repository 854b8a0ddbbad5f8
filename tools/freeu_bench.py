"""What FreeU (``pipe.enable_freeu``) costs on one box: the base pipeline, fp16, 512 x 640, DPM-Solver++-20, one image -- the same tree and
process with the switch on (s1 0.9, s2 0.2, b1 1.5, b2 1.6) against the switch off.  Prints one JSON line and, with --out, writes it to a
file (profiles/freeu_bench.json).

    python tools/freeu_bench.py [--reps 5] [--out profiles/freeu_bench.json]

The repeats are INTERLEAVED (off, on, off, on ... with the order swapping every round) so that clock and thermal drift lands on both arms
alike.  ms per step = a pipeline call to latents (garment UNet included, no VAE decode) over its step count, median [min - max] over the
repeats.  The bar is the off arm of the same run: six of about 500 launches per step become slightly heavier, and the expectation to confirm
or refute is that the on arm's median lies inside the off arm's own min - max spread.  ``rel_rms_vs_off`` is the distance of the final
latents from the switch-off arm's: the weights are synthetic, so it documents that the switch really computes something else and says
NOTHING about image quality on a real checkpoint."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FREEU = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from imagdressing_amd import ops
    from imagdressing_amd import scheduler as S
    from tools.deepcache_bench import inputs, spread
    dev, dtype = torch.device("cuda", 0), torch.float16
    pipe = bench.build_pipeline(dev, dtype, 0)
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
              num_images_per_prompt=1, output_type="latent", **inputs(1, args.width, args.height, dev, dtype))

    def call(on):
        pipe.scheduler = S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
        if on:
            pipe.enable_freeu(**FREEU)
        else:
            pipe.disable_freeu()
        n0 = ops.FREEU_COUNTER["launches"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(num_inference_steps=args.steps, **kw).images
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out, ops.FREEU_COUNTER["launches"] - n0

    outs, launches, times = {}, {}, {False: [], True: []}
    for on in (False, True):                                   # warm-up: kernel selection, caches
        _, out, launches[on] = call(on)
        outs[on] = out.float()
    for rep in range(args.reps):
        for on in ((False, True) if rep % 2 == 0 else (True, False)):
            times[on].append(call(on)[0])
    pipe.disable_freeu()
    d = outs[True] - outs[False]
    off, on = spread(times[False]), spread(times[True])
    res = dict(tool="freeu_bench", width=args.width, height=args.height, dtype="fp16", sampler="dpmpp_2m", steps=args.steps, reps=args.reps,
               device=torch.cuda.get_device_name(dev), freeu=FREEU,
               note="synthetic weights: rel_rms_vs_off documents the mechanism and says nothing about image quality",
               ms_per_step=dict(off=off, on=on), freeu_launches_per_call=dict(off=launches[False], on=launches[True]),
               on_over_off_median=round(on["median"] / off["median"], 4),
               on_median_inside_off_spread=bool(off["min"] <= on["median"] <= off["max"]),
               finite=bool(torch.isfinite(outs[True]).all().item()),
               rel_rms_vs_off=float(d.pow(2).mean().sqrt() / outs[False].pow(2).mean().sqrt()))
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
