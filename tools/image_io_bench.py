"""What the image work around the sampling loop costs, host route against device route (``enable_device_image_io``).

    python tools/image_io_bench.py [--requests 1,4] [--repeats 5] [--steps 20] [--out profiles/image_io_bench.json]

Workload: the ControlNet pipeline at 512 x 640 with DPM-Solver++ (20 steps), R = 1 and R = 4 requests in one call; every request brings a
garment, a pose and a face image as 768 x 1024 PIL images.  Per call the front end makes, per request, the pose tensor of the ControlNet
(Lanczos to 512 x 640, the pipeline's own ``_image_tensor``), the garment tensor of the VAE encoder (Lanczos, [-1, 1]) and the CLIP pixels
of garment and face (bicubic short edge 224, centre crop, normalise); the back end is ``_decode`` of the R final latents to uint8.

Two arms, interleaved repeat by repeat in ONE process on one device (arm order alternates):
  host    the default route of THIS tree with the switch off (the parent commit's lines as long as no line of the default path
          changes; recorded in the JSON as "same-tree default route"): Pillow resizes on one thread, fp32
          copies, ``nchw_to_nhwc8``, fp32 NCHW read-back; the CLIP pixels by the same steps as ``CLIPImageProcessor`` (Pillow bicubic,
          crop, numpy normalise, upload)
  device  ``enable_device_image_io()`` and ``DeviceImageProcessor.clip_preprocess``
Times are host wall time between device-wide syncs: ``pre`` (all front-end work of a call), ``post`` (``_decode``), ``call`` (front end +
pipeline call including decode).  The JSON holds every repeat, median, min and max per arm; outputs of the two arms are compared bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def host_clip_pixels(images, device, dtype, size=224):
    """CLIPImageProcessor's steps on the CPU: bicubic short-edge resize, centre crop, /255, normalise, channels first"""
    from PIL import Image
    from imagdressing_amd.image import CLIP_MEAN, CLIP_STD
    mean, std = np.asarray(CLIP_MEAN, np.float32), np.asarray(CLIP_STD, np.float32)
    out = []
    for im in images:
        im = im.convert("RGB")
        w, h = im.size
        nh, nw = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
        im = im.resize((nw, nh), resample=Image.BICUBIC)
        top, left = (nh - size) // 2, (nw - size) // 2
        a = np.asarray(im, dtype=np.float32)[top:top + size, left:left + size] / 255.0
        out.append(((a - mean) / std).transpose(2, 0, 1))
    return torch.from_numpy(np.stack(out)).to(device=device, dtype=dtype)


def summary(xs):
    return dict(median_ms=round(1e3 * statistics.median(xs), 3), min_ms=round(1e3 * min(xs), 3), max_ms=round(1e3 * max(xs), 3),
                all_ms=[round(1e3 * x, 3) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", default="1,4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_io_bench.json"))
    args = ap.parse_args()
    from PIL import Image
    import bench
    from imagdressing_amd import ops, unet as E
    from imagdressing_amd.dressing_sd.pipelines._base import to_image_tensor
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline_controlnet import IMAGDressing_v1
    from imagdressing_amd.image import DeviceImageProcessor
    from imagdressing_amd.scheduler import DPMSolverMultistepScheduler
    from imagdressing_amd.vae import AutoencoderKL
    dev = torch.device("cuda", 0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    base = bench.build_pipeline(dev, dtype, 0)
    sch = DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    pipe = IMAGDressing_v1(vae=AutoencoderKL.random_init(seed=5, device=dev, dtype=dtype), reference_unet=base.reference_unet, unet=base.unet,
                           tokenizer=None, text_encoder=None, controlnet=E.ControlNetModel.random_init(seed=1, device=dev, dtype=dtype),
                           image_encoder=None, ImgProj=base.ImgProj, scheduler=sch)
    proc = DeviceImageProcessor(dev, dtype)
    rng = np.random.default_rng(11)
    result = dict(tool="image_io_bench", device=torch.cuda.get_device_name(dev), dtype=args.dtype, width=args.width, height=args.height,
                  sampler="DPM-Solver++ 2M", steps=args.steps,
                  arms=dict(host="same-tree default route (switch off)", device="enable_device_image_io + DeviceImageProcessor.clip_preprocess"), source_image="768 x 1024 RGB", repeats=args.repeats, runs={})
    for R in [int(v) for v in args.requests.split(",")]:
        def pil():
            return Image.fromarray(rng.integers(0, 256, size=(1024, 768, 3), dtype=np.uint8))
        garment, pose, face = [pil() for _ in range(R)], [pil() for _ in range(R)], [pil() for _ in range(R)]
        gen = torch.Generator().manual_seed(5)
        lh, lw = args.height // 8, args.width // 8
        fixed = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=args.width, height=args.height,
                     num_inference_steps=args.steps, guidance_scale=[5.0, 6.5, 7.5, 9.0][:R] if R > 1 else 7.5, output_type="np",
                     prompt_embeds=(torch.randn(R, 77, 768, generator=gen) * 0.5).to(dev),
                     negative_prompt_embeds=(torch.randn(R, 77, 768, generator=gen) * 0.5).to(dev),
                     ref_clip_hidden_states=(torch.randn(R, 257, 1280, generator=gen) * 0.5).to(device=dev, dtype=dtype),
                     ref_image_latents=torch.randn(R, 4, lh, lw, generator=gen).to(dev), latents=torch.randn(R, 4, lh, lw, generator=gen).to(dev),
                     controlnet_conditioning_scale=[0.8] * R if R > 1 else 0.8)
        final = torch.randn(R, 4, lh, lw, generator=gen).to(dev)

        def front(device_io, with_pose=True):
            """every tensor the call needs from the 3 R PIL images; ``with_pose=False`` inside a whole call, where the pipeline makes
            the pose tensor itself"""
            pipe.enable_device_image_io(device_io)
            size = (args.height, args.width)
            if not with_pose:
                if device_io:
                    return dict(garment=proc.preprocess(garment, size=size, out="nchw", normalize=True).to(dtype),
                                clip=proc.clip_preprocess(garment + face))
                return dict(garment=to_image_tensor(garment, dev, normalize=True, size=size).to(dtype),
                            clip=host_clip_pixels(garment + face, dev, dtype))
            if device_io:
                return dict(pose=pipe._image_tensor(pose, dev, normalize=False, size=size, layout="nhwc8")[0],
                            garment=proc.preprocess(garment, size=size, out="nchw", normalize=True).to(dtype),
                            clip=proc.clip_preprocess(garment + face))
            return dict(pose=E.nchw_to_nhwc8(to_image_tensor(pose, dev, normalize=False, size=size), dtype),
                        garment=to_image_tensor(garment, dev, normalize=True, size=size).to(dtype),
                        clip=host_clip_pixels(garment + face, dev, dtype))

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        def whole(device_io):
            f = front(device_io, with_pose=False)
            return f, pipe(pose_image=pose if R > 1 else pose[0], **fixed).images

        times = {arm: dict(pre=[], post=[], call=[]) for arm in ("host", "device")}
        outs = {}
        for rep in range(args.repeats + 1):                      # repeat 0 warms both arms up and is dropped
            for arm in (("host", "device") if rep % 2 == 0 else ("device", "host")):
                io = arm == "device"
                t_pre, f = timed(lambda: front(io))
                t_post, img = timed(lambda: pipe._decode(final, "np").images)
                t_call, (f2, full) = timed(lambda: whole(io))
                outs[arm] = dict(f, post=img, full=full)
                if rep:
                    times[arm]["pre"].append(t_pre)
                    times[arm]["post"].append(t_post)
                    times[arm]["call"].append(t_call)
        pipe.disable_device_image_io()
        same = {k: bool(torch.equal(torch.as_tensor(outs["host"][k]), torch.as_tensor(outs["device"][k]))) for k in ("pose", "garment", "post", "full")}
        clip_diff = float((outs["host"]["clip"].float() - outs["device"]["clip"].float()).abs().max())
        run = {arm: {k: summary(v) for k, v in times[arm].items()} for arm in times}
        run["bit_identical"] = same
        run["clip_pixels_max_abs_diff"] = clip_diff
        run["call_median_speedup"] = round(run["host"]["call"]["median_ms"] / run["device"]["call"]["median_ms"], 4)
        run["image_io_launches_per_device_call"] = "R pose + R garment + 2R CLIP resamples, 1 pack"
        result["runs"][f"R{R}"] = run
        print(f"R={R}: " + json.dumps({arm: {k: run[arm][k]["median_ms"] for k in ("pre", "post", "call")} for arm in ("host", "device")})
              + f" identical={same} clip_diff={clip_diff:.2e}", flush=True)
    ops.clear_workspaces()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(tool="image_io_bench", out=os.path.relpath(args.out, ROOT),
                          call_median_speedup={k: v["call_median_speedup"] for k, v in result["runs"].items()})), flush=True)


if __name__ == "__main__":
    main()
