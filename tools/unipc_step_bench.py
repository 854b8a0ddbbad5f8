"""What UniPC's fused-step switch costs on one box: the base pipeline at 512 x 640, one image, UniPC-20, synthetic weights, call time to
latents with the garment UNet included (no VAE decode).  Prints one JSON line and, with --out, writes it to a file
(profiles/unipc_step_bench.json).

    python tools/unipc_step_bench.py [--steps 20] [--reps 5] [--dtype fp16] [--out profiles/unipc_step_bench.json]

One process, one tree, INTERLEAVED repeats (one run of every arm per round, the order rotating), median [min - max]:
  * ``off_eager``: the switch off -- three ``imd_lincomb`` launches and the identity ``imd_ddim_cfg_step`` per step, the route of every
    earlier commit;
  * ``on_eager`` / ``on_graph``: ``scheduler.enable_fused_step()`` -- one ``imd_unipc_step`` per step -- eagerly and under
    ``enable_step_graph``;
  * ``on_batched_4`` against ``on_solo_x4``: four requests with four different guidance scales in ONE call against four solo calls;
  * ``session_unipc`` against ``session_dpmpp_2m``: ms per ``step()`` of a 4-slot session with four requests running, UniPC on the fused
    step against the DPM-Solver++ session of tools/session_bench.py (same measurement: synchronised, the admitting step left out).
THE GATE: one launch replaces four among ~500, so no speed-up is promised -- the switch must cost nothing: ``on_eager``'s median ms per
step may not lie above ``off_eager``'s MAXIMUM over the repeats of the same run (the parent route's own run-to-run spread is the margin).
The graph, batched and session arms are recorded, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


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
    import session_bench as SB
    from imagdressing_amd import scheduler as S
    dev = torch.device("cuda", 0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    pipe = bench.build_pipeline(dev, dtype, 0)
    SB.STEPS = args.steps
    inp = SB.Inputs(args.width, args.height, dev, dtype)

    def unipc(on):
        return S.UniPCMultistepScheduler(fused_step=on, **KW)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, all(bool(torch.isfinite(o).all().item()) for o in outs)

    def call_arm(on, graph, ks):
        def run():
            pipe.scheduler = unipc(on)
            pipe.enable_step_graph(graph)
            try:
                return timed(lambda: [pipe(**inp.call_kwargs(ks)).images])
            finally:
                pipe.enable_step_graph(False)
        return run

    def solo_x4():
        pipe.scheduler = unipc(True)
        return timed(lambda: [pipe(**inp.call_kwargs([k])).images for k in range(4)])

    def session_arm(make):
        def run():
            pipe.scheduler = make()
            ts = SB.session_steps(pipe, inp, 4)
            return statistics.median(ts), True          # per-step seconds, synchronised; the step that admits is left out
        return run
    arms = {"off_eager": call_arm(False, False, [0]), "on_eager": call_arm(True, False, [0]), "on_graph": call_arm(True, True, [0]),
            "on_batched_4": call_arm(True, False, range(4)), "on_solo_x4": solo_x4,
            "session_unipc": session_arm(lambda: unipc(True)), "session_dpmpp_2m": session_arm(SB.scheduler)}
    names = list(arms)
    finite = {n: arms[n]()[1] for n in names}                         # warm-up: kernel selection, caches, graph capture
    times = {n: [] for n in names}
    for rep in range(args.reps):
        for n in names[rep % len(names):] + names[:rep % len(names)]:
            times[n].append(arms[n]()[0])
    res = dict(tool="unipc_step_bench", width=args.width, height=args.height, dtype=args.dtype, steps=args.steps, reps=args.reps,
               device=torch.cuda.get_device_name(dev), arms={})
    for n in ("off_eager", "on_eager", "on_graph"):
        ts = times[n]
        res["arms"][n] = dict(ms_per_call=SB.spread(ts), ms_per_step=SB.spread([t / args.steps for t in ts]), finite=finite[n])
    for n in ("on_batched_4", "on_solo_x4"):
        res["arms"][n] = dict(ms_for_4_requests=SB.spread(times[n]), finite=finite[n])
    for n in ("session_unipc", "session_dpmpp_2m"):
        res["arms"][n] = dict(ms_per_session_step_4of4=SB.spread(times[n]), finite=finite[n])
    a = res["arms"]
    res["batched_4_over_solo_x4"] = round(a["on_batched_4"]["ms_for_4_requests"]["median"] / a["on_solo_x4"]["ms_for_4_requests"]["median"], 4)
    res["gate"] = dict(on_eager_ms_per_step_median=a["on_eager"]["ms_per_step"]["median"], off_eager_ms_per_step_max=a["off_eager"]["ms_per_step"]["max"],
                       holds=a["on_eager"]["ms_per_step"]["median"] <= a["off_eager"]["ms_per_step"]["max"])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
