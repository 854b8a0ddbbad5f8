"""What ``guidance_rescale`` costs on one box.  Prints one JSON line and, with --out, writes it to a file
(profiles/guidance_rescale_bench.json).

    python tools/guidance_rescale_bench.py [--reps 5] [--out profiles/guidance_rescale_bench.json]

1. The kernel alone (``imd_guidance_rescale``, one workgroup per latent row) at HW = 5120 (512 x 640) and 20480 (1024 x 1280), B = 1
   and 4: device events around ``--iters`` back-to-back launches, us per launch.
2. The base pipeline, fp16, 512 x 640, DPM-Solver++-20, one image and four requests, four arms: the keyword absent, 0, 0.7, and (four
   requests) [0, 0.7, 0, 0.7].  ms per step = a pipeline call to latents over its step count.
Every figure is the median [min - max] over ``--reps`` repeats, the arms INTERLEAVED (their order swapping every round) so that clock and
thermal drift lands on all of them alike.

No speed-up is claimed.  ``library_calls`` counts the calls of every entry point of the library during one pipeline call (a counting
proxy around the loaded library, in a run of its own, not in the timed ones): absent and 0 must show the same counts, and 0.7 exactly
``steps`` calls of imd_guidance_rescale more.  ``expected_on_ms_per_step`` = the off median + the standalone kernel time;
``on_exceeds_off_max_by_more_than_the_kernel`` says whether the 0.7 median lies above the off arm's maximum by more than that."""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class CountingLib:
    """the loaded library with every call counted by entry point"""

    def __init__(self, lib):
        self._lib, self.counts = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.counts[name] += 1
            return fn(*a)
        return call


def kernel_alone(HW, B, iters, reps, dev):
    from imagdressing_amd import ops
    gen = torch.Generator().manual_seed(HW + B)
    eps = (torch.randn(2 * B, HW, 4, generator=gen) + 0.3).to(dev)
    g = 7.5 if B == 1 else torch.tensor([5.0, 6.5, 7.5, 9.0][:B]).to(dev)
    phi = 0.7 if B == 1 else torch.full((B,), 0.7).to(dev)
    for _ in range(10):
        ops.guidance_rescale(eps, guidance=g, rescale=phi)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            ops.guidance_rescale(eps, guidance=g, rescale=phi)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / iters)
    return ts


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
    from imagdressing_amd import _lib
    from imagdressing_amd import scheduler as S
    from tools.deepcache_bench import inputs, spread
    dev, dtype = torch.device("cuda", 0), torch.float16
    res = dict(tool="guidance_rescale_bench", width=args.width, height=args.height, dtype="fp16", sampler="dpmpp_2m", steps=args.steps,
               reps=args.reps, device=torch.cuda.get_device_name(dev), kernel_us={}, pipeline={})
    # interleaved like the pipeline arms: every shape once per round
    shapes = [(HW, B) for HW in (5120, 20480) for B in (1, 4)]
    per_shape = {s: [] for s in shapes}
    for rep in range(args.reps):
        for s in (shapes if rep % 2 == 0 else shapes[::-1]):
            per_shape[s] += kernel_alone(s[0], s[1], args.iters, 1, dev)
    for (HW, B), ts in per_shape.items():
        res["kernel_us"][f"HW{HW}_B{B}"] = spread(ts, scale=1e6)

    pipe = bench.build_pipeline(dev, dtype, 0)
    real = _lib.load()
    for R in (1, 4):
        kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
                  num_images_per_prompt=1, output_type="latent", **inputs(R, args.width, args.height, dev, dtype))
        arms = {"absent": {}, "zero": dict(guidance_rescale=0.0), "on": dict(guidance_rescale=0.7)}
        if R == 4:
            arms["mixed"] = dict(guidance_rescale=[0.0, 0.7, 0.0, 0.7])

        def call(arm):
            pipe.scheduler = S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                           beta_schedule="scaled_linear")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(num_inference_steps=args.steps, **kw, **arms[arm]).images
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps, out

        outs, counts, times = {}, {}, {a: [] for a in arms}
        for arm in arms:                                       # warm-up, then one counted call (not timed)
            call(arm)
            _lib._lib = proxy = CountingLib(real)
            try:
                outs[arm] = call(arm)[1].float()
            finally:
                _lib._lib = real
            counts[arm] = dict(proxy.counts)
        names = list(arms)
        for rep in range(args.reps):
            for arm in (names if rep % 2 == 0 else names[::-1]):
                times[arm].append(call(arm)[0])
        sp = {a: spread(times[a]) for a in arms}
        extra = {a: {k: v - counts["absent"].get(k, 0) for k, v in counts[a].items() if v != counts["absent"].get(k, 0)} for a in arms}
        kern_ms = res["kernel_us"][f"HW{(args.width // 8) * (args.height // 8)}_B{R}"]["median"] * 1e-3 \
            if f"HW{(args.width // 8) * (args.height // 8)}_B{R}" in res["kernel_us"] else None
        d = outs["on"] - outs["absent"]
        res["pipeline"][f"requests_{R}"] = dict(
            ms_per_step=sp, library_calls_per_call=dict(absent=sum(counts["absent"].values())),
            library_calls_beyond_absent=extra, zero_same_calls_as_absent=bool(counts["zero"] == counts["absent"]),
            zero_bit_identical_to_absent=bool(torch.equal(outs["zero"], outs["absent"])),
            on_over_off_median=round(sp["on"]["median"] / sp["absent"]["median"], 4),
            expected_on_ms_per_step=None if kern_ms is None else round(sp["absent"]["median"] + kern_ms, 3),
            on_exceeds_off_max_by_more_than_the_kernel=None if kern_ms is None else bool(sp["on"]["median"] > sp["absent"]["max"] + kern_ms),
            finite=bool(torch.isfinite(outs["on"]).all().item()),
            rel_rms_on_vs_absent=float(d.pow(2).mean().sqrt() / outs["absent"].pow(2).mean().sqrt()))
    res["note"] = "synthetic weights: rel_rms_on_vs_absent documents the mechanism and says nothing about image quality"
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
