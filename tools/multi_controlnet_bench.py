"""Several ControlNets per call (``controlnet=[a, b]``): what the mix launch and the second net cost.

    python tools/multi_controlnet_bench.py [--requests 4] [--reps 5] [--steps 20] [--out profiles/multi_controlnet_bench.json]
    python tools/multi_controlnet_bench.py --only-a --record-a FILE        # arm (a) alone: its library calls and a digest of its bits

One MI355X, one process, 512 x 640, DPM-Solver++-20, full-width random-init SD1.5 weights; every figure is the median [min - max] over
``reps`` repeats with the arms INTERLEAVED after one warm-up of each.  No speed-up is claimed; the figures are recorded as found.

1. The kernel alone (``imd_residual_mix_rows``) at the 13 residual shapes, 2 R batch rows, K = 2 and 3 sources: us per launch (HIP
   events around ``iters`` back-to-back launches), bytes moved (K sources read + one written), TB/s.  Back-to-back launches find part
   of their operands in the Infinity Cache; a launch between a ControlNet and a UNet forward does not.  The bar is what the launch
   REPLACES, built in the same run from existing entry points: one in-place ``imd_residual_scale_rows`` per net, then 13 (K - 1)
   element-wise ``imd_add`` launches.  ``mix_median_below_composition_min`` says whether the bar was met.
2. The ControlNet pipeline, fp16, R requests, four arms:
     (a) one net -- today's call        (b) two nets, both open        (c) two nets, net 1 with the window [0, 0.5], eager
     (d) the same as (c) under ``enable_step_graph``
   and the call without a ControlNet, from which ``controlnet_forward_seconds`` = ((a) - none) / steps.  Expected: (b) = (a) + steps x
   (a ControlNet forward + the mix launch); (c) between (a) and (b).  Expectation and measurement stand side by side.
   ``--record-a`` / ``--compare-a``: the library calls per entry point and a digest of the bits of arm (a), written to / compared with
   a file, so that the same arm can be run on another build of the library and the package.
3. bf16: arms (a) and (b), to confirm that it behaves alike."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from control_rows_bench import residual_shapes, spread  # noqa: E402


def timed(fns, iters, reps):
    """{name: fn} -> {name: [us per call]}: HIP events around ``iters`` back-to-back calls, arms interleaved, order alternating"""
    us = {a: [] for a in fns}
    for fn in fns.values():
        for _ in range(5):
            fn()
    for rep in range(reps):
        for a in (list(fns) if rep % 2 == 0 else list(fns)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fns[a]()
            e1.record()
            torch.cuda.synchronize()
            us[a].append(e0.elapsed_time(e1) * 1e3 / iters)
    return us


def kernel_alone(dtype, rows, h, w, K, iters, reps):
    from imagdressing_amd import ops
    shapes = residual_shapes(h, w)
    srcs = [[(torch.randn(rows, *s, device="cuda") * 0.5).to(dtype) for s in shapes] for _ in range(K)]
    work = [[t.clone() for t in src] for src in srcs]          # the composition scales in place: its own copies, which drift towards 0
    dst = [torch.empty_like(t) for t in srcs[0]]
    per_row = sum(t[0].numel() for t in dst) * 2
    scales = torch.full((K, rows), 0.999, device="cuda")
    scales[:, ::2] = 0.501

    def mix():
        ops.residual_mix_rows(srcs, scales, out=dst)

    def composition():
        for k in range(K):
            ops.residual_scale_rows(work[k], scales[k])
        for k in range(1, K):
            for a, b in zip(work[0], work[k]):
                ops.add(a, b, out=a)
    us = timed({"mix_rows": mix, "scale_rows_then_adds": composition}, iters, reps)
    moved = (K + 1) * per_row * rows
    med = statistics.median(us["mix_rows"])
    return dict(sources=K, rows=rows, segments=len(dst), bytes_per_row=per_row, bytes_moved=moved,
                launches_replaced=K + len(dst) * (K - 1), us_per_launch={a: spread(v, 2) for a, v in us.items()},
                tb_per_s=round(moved / med / 1e6, 3), mix_median_below_composition_min=bool(med < min(us["scale_rows_then_adds"])))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=4)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only-a", action="store_true", help="arm (a) alone: no name this tool uses there is newer than the per-request scales")
    ap.add_argument("--record-a", default=None, help="write the library calls and the digest of arm (a) to this file")
    ap.add_argument("--compare-a", default=None, help="compare arm (a) with a file written by --record-a")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_controlnet_bench.json"))
    args = ap.parse_args()
    import bench
    from guidance_rescale_bench import CountingLib
    from imagdressing_amd import _lib
    from imagdressing_amd import scheduler as S
    from imagdressing_amd import unet as E
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    dev = torch.device("cuda", 0)
    R, W, H = args.requests, args.width, args.height
    res = dict(tool="multi_controlnet_bench", device=torch.cuda.get_device_name(dev), requests=R, width=W, height=H, sampler="DPM-Solver++",
               steps=args.steps, reps=args.reps, note="synthetic weights: the figures say nothing about image quality", results={})
    if not args.only_a:
        res["kernel"] = {f"{name}_K{K}": kernel_alone(dt, 2 * R, H // 8, W // 8, K, args.iters, args.reps)
                         for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)) for K in (2, 3)}
    for dname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        if args.only_a and dname != "fp16":
            continue
        base = bench.build_pipeline(dev, dt, 0)
        nets = [E.ControlNetModel.random_init(seed=9 + 2 * k, device=dev, dtype=dt) for k in range(1 if args.only_a else 2)]

        def pipeline(controlnet):
            return IMAGDressing_v1(vae=None, reference_unet=base.reference_unet, unet=base.unet, tokenizer=None, text_encoder=None,
                                   controlnet=controlnet, image_encoder=None, ImgProj=base.ImgProj,
                                   scheduler=S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                                           beta_schedule="scaled_linear"))
        one = pipeline(nets[0])
        two = None if args.only_a else pipeline(nets)
        g = torch.Generator().manual_seed(77)
        rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale        # noqa: E731
        batched = dict(prompt_embeds=rn(R, 77, 768, scale=0.5).to(dev), negative_prompt_embeds=rn(R, 77, 768, scale=0.5).to(dev),
                       ref_clip_hidden_states=rn(R, 257, 1280, scale=0.5).to(device=dev, dtype=dt), ref_image_latents=rn(R, 4, H // 8, W // 8).to(dev),
                       latents=rn(R, 4, H // 8, W // 8).to(dev))
        poses = [torch.rand(R, 3, H, W, generator=g).to(dev) for _ in range(2)]
        common = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=W, height=H, num_inference_steps=args.steps,
                      num_images_per_prompt=1, output_type="latent", guidance_scale=[5.0, 6.5, 7.5, 9.0, 6.0, 8.0, 5.5, 7.0][:R], **batched)

        def arm_a():
            return one(**common, pose_image=poses[0], controlnet_conditioning_scale=0.8).images

        def arm_none():
            return one(**common, pose_image=None).images

        def arm_b():
            return two(**common, pose_image=poses, controlnet_conditioning_scale=[0.8, 0.6]).images

        def arm_c():
            return two(**common, pose_image=poses, controlnet_conditioning_scale=[0.8, 0.6], control_guidance_end=[1.0, 0.5]).images

        def arm_d():
            two.enable_step_graph(True)
            try:
                return arm_c()
            finally:
                two.enable_step_graph(False)

        if args.only_a:
            arms = (("a_one_net", arm_a),)
        elif dname == "fp16":
            arms = (("a_one_net", arm_a), ("none", arm_none), ("b_two_nets", arm_b), ("c_two_nets_net1_half", arm_c),
                    ("d_two_nets_net1_half_step_graph", arm_d))
        else:
            arms = (("a_one_net", arm_a), ("b_two_nets", arm_b))
        outs, times = {}, {n: [] for n, _ in arms}
        real, counts = _lib.load(), {}
        for n, fn in arms:          # per arm, (a) first: one warm-up (kernel selection, workspaces), then one counted call, not timed --
            outs[n] = fn()          # the library calls per entry point; arm (a) is counted in the process state ``--only-a`` counts it in
            torch.cuda.synchronize()
            if n.endswith("step_graph"):
                continue
            _lib._lib = proxy = CountingLib(real)
            try:
                fn()
            finally:
                _lib._lib = real
            counts[n] = dict(proxy.counts)
        for rep in range(1 if args.only_a else args.reps):
            for n, fn in (arms if rep % 2 == 0 else arms[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[n] = fn()
                torch.cuda.synchronize()
                times[n].append(time.perf_counter() - t0)
        med = {n: statistics.median(v) for n, v in times.items()}
        a_record = dict(library_calls=counts["a_one_net"], sha256=digest(outs["a_one_net"]))
        out = dict(seconds_per_arm={n: spread(v) for n, v in times.items()}, ms_per_step={n: round(m / args.steps * 1e3, 3) for n, m in med.items()},
                   arm_a=a_record, finite=bool(all(torch.isfinite(o).all().item() for o in outs.values())))
        if dname == "fp16" and args.record_a:
            with open(args.record_a, "w") as f:
                f.write(json.dumps(a_record, indent=1, sort_keys=True) + "\n")
        if dname == "fp16" and args.compare_a and os.path.isfile(args.compare_a):
            other = json.load(open(args.compare_a))
            out["arm_a_against_the_other_build"] = dict(same_library_calls=bool(other["library_calls"] == a_record["library_calls"]),
                                                        same_bits=bool(other["sha256"] == a_record["sha256"]))
        if not args.only_a:
            beyond = {k: v - counts["a_one_net"].get(k, 0) for k, v in counts["b_two_nets"].items() if v != counts["a_one_net"].get(k, 0)}
            out.update(b_over_a=round(med["b_two_nets"] / med["a_one_net"], 3), mix_launches_of_b=beyond.get("imd_residual_mix_rows", 0),
                       a_makes_no_mix_launch=bool("imd_residual_mix_rows" not in counts["a_one_net"]))
            if dname == "fp16":
                kern_s = res["kernel"]["fp16_K2"]["us_per_launch"]["mix_rows"]["median"] * 1e-6
                fwd = (med["a_one_net"] - med["none"]) / args.steps
                out.update(controlnet_forward_seconds=round(fwd, 5),
                           expected_b_seconds=round(med["a_one_net"] + args.steps * (fwd + kern_s), 4), measured_b_seconds=round(med["b_two_nets"], 4),
                           expected_c_between_a_and_b=[round(med["a_one_net"], 4), round(med["b_two_nets"], 4)],
                           measured_c_seconds=round(med["c_two_nets_net1_half"], 4),
                           c_lies_between=bool(med["a_one_net"] <= med["c_two_nets_net1_half"] <= med["b_two_nets"]),
                           mix_launches_per_arm={n: c.get("imd_residual_mix_rows", 0) for n, c in counts.items()},
                           graph_over_eager=round(med["d_two_nets_net1_half_step_graph"] / med["c_two_nets_net1_half"], 3),
                           graph_bit_identical_to_eager=bool(torch.equal(outs["d_two_nets_net1_half_step_graph"], outs["c_two_nets_net1_half"])))
        res["results"][dname] = out
        del one, two, base, nets
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out and not args.only_a:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
