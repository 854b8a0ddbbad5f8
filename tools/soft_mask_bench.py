"""What ``soft_mask`` costs on one box.  Prints one JSON line and, with --out, writes it to a file (profiles/soft_mask_bench.json).

    python tools/soft_mask_bench.py [--reps 5] [--out profiles/soft_mask_bench.json]

1. ``imd_soft_mask_rows`` alone at HW = 5120 (512 x 640) and 20480 (1024 x 1280), B = 1 and 4: device events around ``--iters``
   back-to-back launches, us per launch.
2. The inpainting pipeline, fp16, 512 x 640, DPM-Solver++-20, one request and four, the mask a feathered 768 x 1024 "L" image on the
   host image route, three arms: ``soft_mask`` absent, False and True.  ms per step = a pipeline call to latents over its step count.
Every figure is the median [min - max] over ``--reps`` repeats in ONE process, the arms INTERLEAVED (their order swapping every round)
so that clock and thermal drift lands on all of them alike.

3. The release map of one 768 x 1024 mask, made once per request: numpy on the host route, one launch on the device route.
No speed-up is claimed: the bar is the absent arm of the same run.  ``expected_true_ms_per_step`` = the absent median + the standalone
kernel time (n launches over n steps); ``..._with_host_maps`` adds the R host release maps of the call spread over its steps;
``true_median_inside_absent_min_max`` says whether the True arm's median lies inside the absent arm's own spread.  ``library_calls`` counts the calls of every entry point during one pipeline call (a counting proxy around the loaded
library, in a call of its own, not a timed one): absent and False must be equal, True adds exactly ``steps`` calls of
imd_soft_mask_rows -- and, on the device image route (counted as well, not timed), one imd_image_mask_release per mask.
Synthetic weights: what the keyword does to image quality with real weights is unmeasured."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def kernel_alone(HW, B, iters, dev):
    from imagdressing_amd import ops
    rng = np.random.default_rng(HW + B)
    release = torch.from_numpy(rng.integers(0, 21, size=(B, HW)).astype(np.uint16)).to(dev)
    steps = torch.full((B,), 10, dtype=torch.int32, device=dev)
    mask = torch.zeros(B, HW, device=dev)
    for _ in range(10):
        ops.soft_mask_rows(mask, release, steps)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        ops.soft_mask_rows(mask, release, steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def feathered_mask(hw, seed):
    """255 in a torso-sized rectangle, a linear ramp of 96 pixels to 0 around it: uint8 [H0, W0]"""
    H0, W0 = hw
    y, x = np.mgrid[0:H0, 0:W0]
    t, b, l, r = H0 // 4 + 8 * seed, 3 * H0 // 4, W0 // 4, 3 * W0 // 4 - 8 * seed
    d = np.maximum(np.maximum(t - y, y - b), np.maximum(l - x, x - r)).clip(0, 96)
    return (255 - d * 255 // 96).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from PIL import Image
    from deepcache_bench import inputs, spread
    from guidance_rescale_bench import CountingLib
    from imagdressing_amd import _lib
    from imagdressing_amd import scheduler as S
    from imagdressing_amd import unet as E
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet_inpainting import IMAGDressing_v1
    dev, dtype = torch.device("cuda", 0), torch.float16
    W, H = args.width, args.height
    res = dict(tool="soft_mask_bench", width=W, height=H, dtype="fp16", sampler="dpmpp_2m", steps=args.steps, reps=args.reps,
               device=torch.cuda.get_device_name(dev), kernel_us={}, pipeline={})
    shapes = [(HW, B) for HW in (5120, 20480) for B in (1, 4)]
    per_shape = {s: [] for s in shapes}
    for rep in range(args.reps):                               # interleaved like the pipeline arms: every shape once per round
        for s in (shapes if rep % 2 == 0 else shapes[::-1]):
            per_shape[s].append(kernel_alone(s[0], s[1], args.iters, dev))
    for (HW, B), ts in per_shape.items():
        res["kernel_us"][f"HW{HW}_B{B}"] = spread(ts, scale=1e6)

    # the release map of one 768 x 1024 mask, once per request: numpy on the host route, one launch (after the upload) on the device route
    from imagdressing_amd.image import DeviceImageProcessor, mask_as_l, mask_release_reference
    one = Image.fromarray(feathered_mask((1024, 768), 0))
    proc = DeviceImageProcessor(dev, dtype)
    up = proc._upload(one, "L")
    host_ts, dev_ts = [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        mask_release_reference(np.ascontiguousarray(mask_as_l(one)), H // 8, W // 8, args.steps)
        host_ts.append(time.perf_counter() - t0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            proc.mask_release(up, H // 8, W // 8, args.steps)
        b.record()
        torch.cuda.synchronize()
        dev_ts.append(a.elapsed_time(b) * 1e-3 / args.iters)
    res["release_map_768x1024"] = dict(host_numpy_ms=spread(host_ts[1:]), device_launch_us=spread(dev_ts[1:], scale=1e6))

    base = bench.build_pipeline(dev, dtype, 0)
    pipe = IMAGDressing_v1(vae=None, reference_unet=base.reference_unet, unet=base.unet, tokenizer=None, text_encoder=None,
                           controlnet=E.ControlNetModel.random_init(seed=9, device=dev, dtype=dtype), image_encoder=None,
                           ImgProj=base.ImgProj, scheduler=None)
    real = _lib.load()
    gen = torch.Generator().manual_seed(31)
    for R in (1, 4):
        masks = [Image.fromarray(feathered_mask((1024, 768), r)) for r in range(R)]
        kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=W, height=H, num_images_per_prompt=1,
                  output_type="latent", **inputs(R, W, H, dev, dtype))
        kw["noise"] = kw.pop("latents")
        kw.update(image_latents=torch.randn(R, 4, H // 8, W // 8, generator=gen).to(dev),
                  control_image=torch.rand(R, 3, H, W, generator=gen).to(dev), mask_image=masks if R > 1 else masks[0])
        arms = {"absent": {}, "false": dict(soft_mask=False), "true": dict(soft_mask=True)}

        def call(arm):
            pipe.scheduler = S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                           beta_schedule="scaled_linear")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(num_inference_steps=args.steps, **kw, **arms[arm]).images
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps, out

        def counted(arm):
            _lib._lib = proxy = CountingLib(real)
            try:
                out = call(arm)[1].float()
            finally:
                _lib._lib = real
            return out, dict(proxy.counts)

        outs, counts, times = {}, {}, {a: [] for a in arms}
        for arm in arms:                                       # warm-up, then one counted call (not timed)
            call(arm)
            outs[arm], counts[arm] = counted(arm)
        pipe.enable_device_image_io()                          # the device image route: counted, not timed
        try:
            dev_counts = {arm: counted(arm) for arm in ("absent", "true")}
        finally:
            pipe.disable_device_image_io()
        names = list(arms)
        for rep in range(args.reps):
            for arm in (names if rep % 2 == 0 else names[::-1]):
                times[arm].append(call(arm)[0])
        sp = {a: spread(times[a]) for a in arms}

        def beyond(c, ref):
            return {k: v - ref.get(k, 0) for k, v in c.items() if v != ref.get(k, 0)}
        kern_ms = res["kernel_us"][f"HW{(W // 8) * (H // 8)}_B{R}"]["median"] * 1e-3
        d = outs["true"] - outs["absent"]
        res["pipeline"][f"requests_{R}"] = dict(
            ms_per_step=sp, library_calls_per_call=dict(absent=sum(counts["absent"].values())),
            library_calls_true_beyond_absent=beyond(counts["true"], counts["absent"]),
            library_calls_true_beyond_absent_device_route=beyond(dev_counts["true"][1], dev_counts["absent"][1]),
            false_same_calls_as_absent=bool(counts["false"] == counts["absent"]),
            false_bit_identical_to_absent=bool(torch.equal(outs["false"], outs["absent"])),
            device_route_bit_identical_to_host_route=bool(torch.equal(dev_counts["true"][0], outs["true"])),
            true_over_absent_median=round(sp["true"]["median"] / sp["absent"]["median"], 4),
            expected_true_ms_per_step=round(sp["absent"]["median"] + kern_ms, 3),
            expected_true_ms_per_step_with_host_maps=round(
                sp["absent"]["median"] + kern_ms + R * res["release_map_768x1024"]["host_numpy_ms"]["median"] / args.steps, 3),
            true_median_inside_absent_min_max=bool(sp["absent"]["min"] <= sp["true"]["median"] <= sp["absent"]["max"]),
            finite=bool(torch.isfinite(outs["true"]).all().item()),
            rel_rms_true_vs_absent=float(d.pow(2).mean().sqrt() / outs["absent"].pow(2).mean().sqrt()))
    res["note"] = ("synthetic weights: rel_rms_true_vs_absent documents that the keyword computes something else; image quality with real "
                   "weights is unmeasured")
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
