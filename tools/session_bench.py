"""What in-flight batching (``pipe.open_session``) costs and buys on one box: the base pipeline at 512 x 640, DPM-Solver++-20, synthetic
weights, fp16 and bf16.  Prints one JSON line and, with --out, writes it to a file (profiles/session_bench.json).

    python tools/session_bench.py [--reps 5] [--trace-reps 5] [--dtypes fp16,bf16] [--out profiles/session_bench.json]
    python tools/session_bench.py --compact [--ladder 1,2,4] [--out profiles/session_compact_bench.json]      (see the end of this text)

Steady state, INTERLEAVED repeats (one run of every arm per round, the order rotating), median [min - max]:
  * ``batched_call_step``: ms per step of the request-batched call of four requests -- THE BAR (a step callback synchronises and reads
    the wall clock; call 0 left out, it also fills the processors' K / V caches);
  * ``session_step_4of4`` / ``session_step_1of4``: ms per ``step()`` of a 4-slot session with four / one request running, synchronised the
    same way, steps that admit left out;
  * ``admission``: a ``step()`` that admits ONE request into a session whose other three slots run (prompt rows, garment UNet at batch 1,
    time-embedding table, and the K / V refresh of all slots in the forward that follows), and the same minus that run's median plain step.
Arrival trace: 24 requests with seeded exponential inter-arrival times at 0.5x and 0.9x of the measured solo service rate (1 / the
median solo call); a request becomes visible when the wall clock passes its arrival time.  Served (a) by solo calls, FIFO, (b) by
request-batched calls of whatever has arrived (up to 4) each time the GPU is free, (c) by one session with 4 slots (steps are launched
one ahead of the GPU, so the host work of a step overlaps the kernels of the previous one like it does inside a pipeline call).  Per
arm: images/s from the first arrival to the last result, mean and worst latency from arrival to latents.

``--compact`` measures the compacting session (``open_session(..., compact=True)``) beside all of the above in ONE run, the arms interleaved
the same way: ms per step with 1, 2, 3, 4 of 4 slots running for the default session, the compacting one and the compacting one on the
``--ladder`` widths; a ``slots=1`` default session (what a width-1 step should cost) and the request-batched call of 1, 2, 3, 4 requests
(what a width-n step should cost); a step that repacks 2 -> 1 against the plain width-1 steps behind it; and the two arrival traces served
by solo calls / batched calls / the default session / the compacting session / the compacting session on the ladder.  The figures of
profiles/session_bench.json for the arms that file has are copied beside the new ones (``parent_commit``)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

STEPS = 20
GUIDANCE = [5.0, 6.5, 7.5, 9.0]


def scheduler():
    from imagdressing_amd import scheduler as S
    return S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


class Inputs:
    """four distinct requests (garment, prompt, latent, guidance); request k of a trace uses entry k % 4"""

    def __init__(self, width, height, device, dtype):
        gen = torch.Generator().manual_seed(2024)
        lh, lw = height // 8, width // 8
        self.width, self.height = width, height
        self.pe = (torch.randn(4, 77, 768, generator=gen) * 0.5).to(device)
        self.ne = (torch.randn(4, 77, 768, generator=gen) * 0.5).to(device)
        self.clip = (torch.randn(4, 257, 1280, generator=gen) * 0.5).to(device=device, dtype=dtype)
        self.refl = torch.randn(4, 4, lh, lw, generator=gen).to(device)
        self.lat = torch.randn(4, 4, lh, lw, generator=gen).to(device)

    def call_kwargs(self, ks):
        i = [k % 4 for k in ks]
        g = [GUIDANCE[j] for j in i]
        return dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=self.width, height=self.height,
                    num_images_per_prompt=1, output_type="latent", num_inference_steps=STEPS, prompt_embeds=self.pe[i], negative_prompt_embeds=self.ne[i],
                    ref_clip_hidden_states=self.clip[i], ref_image_latents=self.refl[i], latents=self.lat[i], guidance_scale=g[0] if len(g) == 1 else g)

    def submit_kwargs(self, k, steps=STEPS):
        j = k % 4
        return dict(num_inference_steps=steps, guidance_scale=GUIDANCE[j], prompt_embeds=self.pe[j:j + 1], negative_prompt_embeds=self.ne[j:j + 1],
                    ref_clip_hidden_states=self.clip[j:j + 1], ref_image_latents=self.refl[j:j + 1], latents=self.lat[j:j + 1], output_type="latent")


def spread(ts, scale=1e3):
    return dict(median=round(scale * statistics.median(ts), 3), min=round(scale * min(ts), 3), max=round(scale * max(ts), 3))


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


# ---- steady state ----
def batched_call_steps(pipe, inp):
    marks = []

    def cb(i, t, z):
        marks.append(sync_clock())
    pipe(callback=cb, **inp.call_kwargs(range(4)))
    return [marks[i] - marks[i - 1] for i in range(1, len(marks))]


def session_steps(pipe, inp, running, slots=4, **open_kw):
    """plain steps of a 4-slot session with ``running`` requests of STEPS steps (the admitting step left out)"""
    out = []
    with pipe.open_session(slots=slots, width=inp.width, height=inp.height, **open_kw) as ses:
        for k in range(running):
            ses.submit(**inp.submit_kwargs(k))
        ses.step()
        for _ in range(STEPS - 1):
            t0 = sync_clock()
            ses.step()
            out.append(sync_clock() - t0)
    return out


def batched_call_steps_of(pipe, inp, R):
    marks = []

    def cb(i, t, z):
        marks.append(sync_clock())
    pipe(callback=cb, **inp.call_kwargs(range(R)))
    return [marks[i] - marks[i - 1] for i in range(1, len(marks))]


def repack_step(pipe, inp, **open_kw):
    """-> (seconds of the step that repacks 2 -> 1 -- the survivor's rows re-laid, the step-invariant caches refreshed --, median plain
    width-1 step behind it) in a compacting 4-slot session: two requests of STEPS and STEPS / 2 steps"""
    with pipe.open_session(slots=4, width=inp.width, height=inp.height, compact=True, **open_kw) as ses:
        ses.submit(**inp.submit_kwargs(0))
        ses.submit(**inp.submit_kwargs(1, steps=STEPS // 2))
        for _ in range(STEPS // 2):
            ses.step()
        assert ses.width == 2 and ses.rows == [0, None]
        t0 = sync_clock()
        ses.step()
        t = sync_clock() - t0
        assert ses.width == 1 and ses.repacks == 1
        plain = []
        for _ in range(STEPS // 2 - 2):
            t0 = sync_clock()
            ses.step()
            plain.append(sync_clock() - t0)
        return t, statistics.median(plain)


def admission(pipe, inp):
    """-> (seconds of the step that admits one request beside three running ones, median plain step of the same session)"""
    with pipe.open_session(slots=4, width=inp.width, height=inp.height) as ses:
        for k in range(3):
            ses.submit(**inp.submit_kwargs(k, steps=2 * STEPS))
        ses.step()
        plain = []
        for _ in range(6):
            t0 = sync_clock()
            ses.step()
            plain.append(sync_clock() - t0)
        ses.submit(**inp.submit_kwargs(3))
        t0 = sync_clock()
        ses.step()
        return sync_clock() - t0, statistics.median(plain)


# ---- arrival trace ----
def arrivals(n, mean_gap, seed):
    rnd, t, out = random.Random(seed), 0.0, []
    for _ in range(n):
        out.append(t)
        t += rnd.expovariate(1.0 / mean_gap)
    return out


def wait_until(t):
    while True:
        d = t - time.perf_counter()
        if d <= 0:
            return
        time.sleep(min(d, 0.0005))


def summary(arr, fin):
    lat = [f - a for a, f in zip(arr, fin)]
    return dict(images_per_s=len(arr) / (max(fin) - arr[0]), mean_latency_ms=1e3 * statistics.mean(lat), worst_latency_ms=1e3 * max(lat))


def serve_solo(pipe, inp, arr):
    t0, fin = time.perf_counter(), []
    for k, a in enumerate(arr):
        wait_until(t0 + a)
        pipe(**inp.call_kwargs([k]))
        fin.append(sync_clock() - t0)
    return summary(arr, fin)


def serve_batched(pipe, inp, arr):
    t0, fin, k = time.perf_counter(), [], 0
    while k < len(arr):
        wait_until(t0 + arr[k])
        now = time.perf_counter() - t0
        ks = [j for j in range(k, min(k + 4, len(arr))) if arr[j] <= now]
        pipe(**inp.call_kwargs(ks))
        done = sync_clock() - t0
        fin += [done] * len(ks)
        k += len(ks)
    return summary(arr, fin)


def serve_session(pipe, inp, arr, **open_kw):
    fin, k, tickets = [None] * len(arr), 0, {}
    with pipe.open_session(slots=4, width=inp.width, height=inp.height, **open_kw) as ses:
        t0, prev = time.perf_counter(), None
        while any(f is None for f in fin):
            if not tickets and k < len(arr):
                wait_until(t0 + arr[k])
            now = time.perf_counter() - t0
            while k < len(arr) and arr[k] <= now:
                tickets[k] = ses.submit(**inp.submit_kwargs(k))
                k += 1
            wait, prev = prev, torch.cuda.Event()
            done = ses.step()
            prev.record()
            if done:
                stamp = sync_clock() - t0
                for j in [j for j, t in tickets.items() if t in done]:
                    fin[j] = stamp
                    del tickets[j]
            elif wait is not None:
                wait.synchronize()              # at most one step ahead of the GPU
    return summary(arr, fin)


def rotate(items, rep):
    k = rep % len(items)
    return items[k:] + items[:k]


def compact_results(pipe, inp, args, ladder):
    """the --compact measurement of one element type -> dict(steady_state_ms=, arrival_trace=)"""
    for R in (1, 2, 3, 4):                                      # warm-up: kernel selection and workspaces of every batch width
        pipe(**inp.call_kwargs(range(R)))
        session_steps(pipe, inp, R, compact=True)
    session_steps(pipe, inp, 4)
    session_steps(pipe, inp, 1, slots=1)
    arms = {"slots1_session_step": lambda: session_steps(pipe, inp, 1, slots=1)}
    for n in (1, 2, 3, 4):
        arms[f"session_step_{n}of4"] = lambda n=n: session_steps(pipe, inp, n)
        arms[f"compact_step_{n}of4"] = lambda n=n: session_steps(pipe, inp, n, compact=True)
        arms[f"batched_call_step_{n}"] = lambda n=n: batched_call_steps_of(pipe, inp, n)
    arms["ladder_step_3of4"] = lambda: session_steps(pipe, inp, 3, compact=True, widths=ladder)
    names = list(arms) + ["repack"]
    per_run = {a: [] for a in arms}
    rep_t, rep_extra, solo_t = [], [], []
    for rep in range(args.reps):
        for a in rotate(names, rep):
            if a == "repack":
                t, plain = repack_step(pipe, inp)
                rep_t.append(t)
                rep_extra.append(t - plain)
            else:
                per_run[a].append(statistics.median(arms[a]()))
        t0 = sync_clock()
        pipe(**inp.call_kwargs([rep]))
        solo_t.append(sync_clock() - t0)
    steady = {a: spread(v) for a, v in per_run.items()}
    steady["repacking_step_2to1"] = spread(rep_t)
    steady["repack_over_plain_step"] = spread(rep_extra)
    steady["solo_call"] = spread(solo_t)
    steady["ratio_compact_1of4_vs_slots1"] = round(steady["compact_step_1of4"]["median"] / steady["slots1_session_step"]["median"], 4)
    for n in (1, 2, 3, 4):
        steady[f"ratio_compact_{n}of4_vs_batched_call_{n}"] = round(steady[f"compact_step_{n}of4"]["median"] / steady[f"batched_call_step_{n}"]["median"], 4)
    print("# steady: " + json.dumps(steady), file=sys.stderr, flush=True)
    solo = statistics.median(solo_t)
    traces = {}
    servers = [("solo_fifo", serve_solo), ("batched_calls", serve_batched), ("session_4_slots", serve_session),
               ("compact_session_4_slots", lambda p, i, a: serve_session(p, i, a, compact=True)),
               ("compact_session_ladder", lambda p, i, a: serve_session(p, i, a, compact=True, widths=ladder))]
    for load in (0.5, 0.9):
        runs = {n: [] for n, _ in servers}
        for rep in range(args.trace_reps):
            arr = arrivals(args.requests, solo / load, seed=1000 + rep)          # the same trace for every server of a repeat
            for n, fn in rotate(servers, rep):
                runs[n].append(fn(pipe, inp, arr))
        block = {}
        for n, rs in runs.items():
            block[n] = dict(images_per_s=spread([r["images_per_s"] for r in rs], 1.0), mean_latency_ms=spread([r["mean_latency_ms"] for r in rs], 1.0),
                            worst_latency_ms=spread([r["worst_latency_ms"] for r in rs], 1.0))
        traces[f"load_{load}"] = dict(mean_inter_arrival_ms=round(1e3 * solo / load, 3), **block)
        print(f"# load {load}: " + json.dumps(block), file=sys.stderr, flush=True)
    return dict(steady_state_ms=steady, arrival_trace=traces)


def parent_figures(dname):
    """the arms profiles/session_bench.json has in common with the --compact run (measured before sessions could compact)"""
    try:
        with open(os.path.join(ROOT, "profiles", "session_bench.json")) as f:
            old = json.load(f)["results"][dname]
    except (OSError, KeyError, ValueError):
        return None
    keep = ("session_step_4of4", "session_step_1of4", "batched_call_step", "solo_call")
    return dict(steady_state_ms={k: old["steady_state_ms"][k] for k in keep if k in old["steady_state_ms"]},
                arrival_trace={load: {n: v[n]["mean_latency_ms"] for n in ("solo_fifo", "batched_calls", "session_4_slots") if n in v}
                               for load, v in old["arrival_trace"].items()})


def main_compact(args):
    import bench
    from imagdressing_amd import ops
    dev = torch.device("cuda", 0)
    ladder = tuple(int(w) for w in args.ladder.split(","))
    res = dict(tool="session_bench --compact", width=args.width, height=args.height, sampler=f"dpmpp_2m_{STEPS}", reps=args.reps,
               trace_reps=args.trace_reps, trace_requests=args.requests, ladder=list(ladder), device=torch.cuda.get_device_name(dev),
               note="synthetic weights; every arm of a repeat in one process, interleaved, the order rotating; median [min - max]", results={})
    for dname in args.dtypes.split(","):
        dtype = torch.float16 if dname == "fp16" else torch.bfloat16
        pipe = bench.build_pipeline(dev, dtype, 0)
        pipe.scheduler = scheduler()
        inp = Inputs(args.width, args.height, dev, dtype)
        res["results"][dname] = dict(compact_results(pipe, inp, args, ladder), parent_commit=parent_figures(dname))
        del pipe
        ops.clear_workspaces()
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-reps", type=int, default=5)
    ap.add_argument("--requests", type=int, default=24)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compact", action="store_true", help="measure the compacting session beside the other arms (a different result file)")
    ap.add_argument("--ladder", default="1,2,4", help="--compact: the width ladder of the laddered arms")
    args = ap.parse_args()
    if args.compact:
        return main_compact(args)
    import bench
    from imagdressing_amd import ops
    dev = torch.device("cuda", 0)
    res = dict(tool="session_bench", width=args.width, height=args.height, sampler=f"dpmpp_2m_{STEPS}", reps=args.reps, trace_reps=args.trace_reps,
               trace_requests=args.requests, device=torch.cuda.get_device_name(dev), note="synthetic weights", results={})
    for dname in args.dtypes.split(","):
        dtype = torch.float16 if dname == "fp16" else torch.bfloat16
        pipe = bench.build_pipeline(dev, dtype, 0)
        pipe.scheduler = scheduler()
        inp = Inputs(args.width, args.height, dev, dtype)
        for R in (1, 2, 3, 4):                                      # warm-up: kernel selection and workspaces of every batch the traces use
            pipe(**inp.call_kwargs(range(R)))
        session_steps(pipe, inp, 4)
        arms = {"batched_call_step": lambda: batched_call_steps(pipe, inp), "session_step_4of4": lambda: session_steps(pipe, inp, 4),
                "session_step_1of4": lambda: session_steps(pipe, inp, 1)}
        names = list(arms) + ["admission"]
        per_run = {a: [] for a in arms}
        adm, adm_extra, solo_t = [], [], []
        for rep in range(args.reps):
            k = rep % len(names)
            for a in names[k:] + names[:k]:
                if a == "admission":
                    t, plain = admission(pipe, inp)
                    adm.append(t)
                    adm_extra.append(t - plain)
                else:
                    per_run[a].append(statistics.median(arms[a]()))
            t0 = sync_clock()
            pipe(**inp.call_kwargs([rep]))
            solo_t.append(sync_clock() - t0)
        steady = {a: spread(v) for a, v in per_run.items()}
        steady["admitting_step"] = spread(adm)
        steady["admission_over_plain_step"] = spread(adm_extra)
        steady["solo_call"] = spread(solo_t)
        steady["ratio_4of4_vs_batched"] = round(steady["session_step_4of4"]["median"] / steady["batched_call_step"]["median"], 4)
        steady["ratio_1of4_vs_batched"] = round(steady["session_step_1of4"]["median"] / steady["batched_call_step"]["median"], 4)
        print(f"# {dname} steady: " + json.dumps(steady), file=sys.stderr, flush=True)
        solo = statistics.median(solo_t)
        traces = {}
        servers = [("solo_fifo", serve_solo), ("batched_calls", serve_batched), ("session_4_slots", serve_session)]
        for load in (0.5, 0.9):
            runs = {n: [] for n, _ in servers}
            for rep in range(args.trace_reps):
                arr = arrivals(args.requests, solo / load, seed=1000 + rep)          # the same trace for the three servers of a repeat
                k = rep % len(servers)
                for n, fn in servers[k:] + servers[:k]:
                    runs[n].append(fn(pipe, inp, arr))
            block = {}
            for n, rs in runs.items():
                block[n] = dict(images_per_s=spread([r["images_per_s"] for r in rs], 1.0), mean_latency_ms=spread([r["mean_latency_ms"] for r in rs], 1.0),
                                worst_latency_ms=spread([r["worst_latency_ms"] for r in rs], 1.0))
            traces[f"load_{load}"] = dict(mean_inter_arrival_ms=round(1e3 * solo / load, 3), **block)
            print(f"# {dname} load {load}: " + json.dumps(block), file=sys.stderr, flush=True)
        res["results"][dname] = dict(steady_state_ms=steady, arrival_trace=traces)
        del pipe
        ops.clear_workspaces()
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
