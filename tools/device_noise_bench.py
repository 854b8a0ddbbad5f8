"""What ``enable_device_noise`` costs on one box.  Prints one JSON line and, with --out, writes it to a file
(profiles/device_noise_bench.json).

    python tools/device_noise_bench.py [--reps 5] [--out profiles/device_noise_bench.json]

1. The kernel alone (``imd_noise_rows``, one 16-byte store per pixel) at HW = 5120 (512 x 640) and 20480 (1024 x 1280), rows 1 and 4:
   device events around ``--iters`` back-to-back launches, us per launch.
2. The base pipeline, fp16, 512 x 640, Euler-ancestral-20, one image, three arms: the switch off and eager (what the code before this
   switch did: torch.randn per step in the UNet's element type -- the bar), the switch on and eager, the switch on under
   ``enable_step_graph`` (the stochastic step replays only with device noise).  ms per step = a pipeline call to latents over its
   step count.
3. A 4-slot session, full, plain steps: Euler-ancestral with device noise against DPM-Solver++ (deterministic, no noise launch) in the
   same run.  ms per step.
Every figure is the median [min - max] over ``--reps`` repeats, the arms INTERLEAVED (their order swapping every round) so that clock and
thermal drift lands on all of them alike.

No speed-up is claimed.  The condition is ``on_eager_inside_off_spread``: the switch-on eager median lies inside the switch-off arm's own
min - max of the same run; where it does not, the figure stands as measured.  ``library_calls_beyond_off`` counts entry-point calls
of one pipeline call (a counting proxy around the loaded library, in a run of its own, not in the timed ones)."""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SEED = 20261020
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def kernel_alone(HW, rows, iters, dev):
    from imagdressing_amd import ops
    out = torch.empty(rows, HW, 4, dtype=torch.float32, device=dev)
    keys = ops.noise_key_rows([ops.noise_key_row(SEED + r, r, 1) for r in range(rows)], dev)
    for _ in range(10):
        ops.noise_rows(out, keys)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        ops.noise_rows(out, keys)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


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
    from tools.guidance_rescale_bench import CountingLib
    from tools.session_bench import Inputs, sync_clock
    dev, dtype = torch.device("cuda", 0), torch.float16
    res = dict(tool="device_noise_bench", width=args.width, height=args.height, dtype="fp16", sampler="euler_ancestral", steps=args.steps,
               reps=args.reps, device=torch.cuda.get_device_name(dev), kernel_us={}, pipeline={}, session={})

    # 1. the kernel alone, interleaved like the pipeline arms: every shape once per round
    shapes = [(HW, rows) for HW in (5120, 20480) for rows in (1, 4)]
    per_shape = {s: [] for s in shapes}
    for rep in range(args.reps):
        for s in (shapes if rep % 2 == 0 else shapes[::-1]):
            per_shape[s].append(kernel_alone(s[0], s[1], args.iters, dev))
    for (HW, rows), ts in per_shape.items():
        res["kernel_us"][f"HW{HW}_rows{rows}"] = spread(ts, scale=1e6)

    # 2. the base pipeline, Euler-ancestral
    pipe = bench.build_pipeline(dev, dtype, 0)
    real = _lib.load()
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
              num_images_per_prompt=1, output_type="latent", **inputs(1, args.width, args.height, dev, dtype))
    kw.pop("latents")
    # the graph arm runs on a shallow copy (the same models): switching enable_step_graph off between arms would drop the captured
    # step's side stream and its workspaces, and the arm would pay for them again at every call
    pipe_g = copy.copy(pipe).enable_step_graph(True)
    arms = {"off_eager": (pipe, False), "on_eager": (pipe, True), "on_graph": (pipe_g, True)}

    def call(arm):
        p, on = arms[arm]
        p.scheduler = S.EulerAncestralDiscreteScheduler(**KW)
        p.enable_device_noise(on)
        extra = dict(seed=SEED) if on else dict(generator=torch.Generator(dev).manual_seed(SEED))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = p(num_inference_steps=args.steps, **kw, **extra).images
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    try:
        outs, counts, times = {}, {}, {a: [] for a in arms}
        for arm in arms:                                       # warm-up, then one counted call (not timed)
            call(arm)
            _lib._lib = proxy = CountingLib(real)
            try:
                outs[arm] = call(arm)[1].float()
            finally:
                _lib._lib = real
            counts[arm] = dict(proxy.counts)
        graph_ran = getattr(pipe_g, "_last_step_graph", None) is not None
        names = list(arms)
        for rep in range(args.reps):
            for arm in (names if rep % 2 == 0 else names[::-1]):
                times[arm].append(call(arm)[0])
    finally:
        pipe_g.enable_step_graph(False)
        pipe.disable_device_noise()
    sp = {a: spread(times[a]) for a in arms}
    off = counts["off_eager"]
    res["pipeline"] = dict(
        ms_per_step=sp,
        library_calls_beyond_off={a: {k: v - off.get(k, 0) for k, v in counts[a].items() if v != off.get(k, 0)} for a in ("on_eager",)},
        on_eager_over_off_median=round(sp["on_eager"]["median"] / sp["off_eager"]["median"], 4),
        on_graph_over_off_median=round(sp["on_graph"]["median"] / sp["off_eager"]["median"], 4),
        on_eager_inside_off_spread=bool(sp["off_eager"]["min"] <= sp["on_eager"]["median"] <= sp["off_eager"]["max"]),
        on_eager_at_or_below_off_max=bool(sp["on_eager"]["median"] <= sp["off_eager"]["max"]),
        graph_bit_identical_to_eager=bool(torch.equal(outs["on_graph"], outs["on_eager"])), graph_ran=bool(graph_ran),
        finite=bool(torch.isfinite(outs["on_eager"]).all().item()))

    # 3. a full 4-slot session: Euler-ancestral with device noise beside DPM-Solver++
    inp = Inputs(args.width, args.height, dev, dtype)

    def session_steps(name):
        pipe.scheduler = S.EulerAncestralDiscreteScheduler(**KW) if name == "euler_ancestral_device_noise" else S.DPMSolverMultistepScheduler(**KW)
        out = []
        with pipe.open_session(slots=4, width=args.width, height=args.height, device_noise=name == "euler_ancestral_device_noise") as ses:
            for k in range(4):
                skw = inp.submit_kwargs(k, steps=args.steps)
                if ses.device_noise:
                    skw.pop("latents")
                    skw["seed"] = SEED + k
                ses.submit(**skw)
            ses.step()                                     # the admitting step is left out
            for _ in range(args.steps - 1):
                t0 = sync_clock()
                ses.step()
                out.append(sync_clock() - t0)
        return out

    sarms = ["dpmpp_2m", "euler_ancestral_device_noise"]
    stimes = {a: [] for a in sarms}
    for a in sarms:
        session_steps(a)                                   # warm-up
    for rep in range(args.reps):
        for a in (sarms if rep % 2 == 0 else sarms[::-1]):
            ts = session_steps(a)
            stimes[a].append(sum(ts) / len(ts))
    ssp = {a: spread(stimes[a]) for a in sarms}
    res["session"] = dict(slots=4, running=4, ms_per_step=ssp,
                          euler_ancestral_over_dpm_median=round(ssp["euler_ancestral_device_noise"]["median"] / ssp["dpmpp_2m"]["median"], 4),
                          euler_ancestral_inside_dpm_spread=bool(ssp["dpmpp_2m"]["min"] <= ssp["euler_ancestral_device_noise"]["median"] <= ssp["dpmpp_2m"]["max"]))
    res["note"] = ("synthetic weights: nothing here says anything about image quality; the switch-on noise is not torch's stream, is fp32 "
                   "and is cut at 5.77 sigma")
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
