"""What the back end of an inpainting call with ``overlay=True`` costs, host route against device route (``enable_device_image_io``).

    python tools/inpaint_overlay_bench.py [--requests 1,4] [--repeats 5] [--out profiles/inpaint_overlay_bench.json]

Workload: the inpainting pipeline's ``_decode_overlay`` at 512 x 640 -- the VAE decode of the R final latents, then every decoded image
resized with Lanczos to its request's crop box and composited into the request's 768 x 1024 person photo through a feathered mask.
The box (``get_crop_region`` with ``padding_mask_crop=32``) covers roughly half of the photo.  R = 1 and R = 4 requests (own photo,
mask and box each), ``output_type="pil"``.

Two arms, interleaved repeat by repeat in ONE process on one device (arm order alternates), the protocol of tools/image_io_bench.py:
  host    the default route: fp32 NCHW read-back of the decoder's output, then per image ``Image.resize`` (Lanczos), ``paste`` and
          ``Image.composite`` on one host thread
  device  ``enable_device_image_io()``: ``imd_image_pack_u8``, per request one ``imd_image_resample`` and one ``imd_image_overlay``,
          one uint8 copy back.  The photos and masks are on the device already, as after the front end of a real call.
Times are host wall time between device-wide syncs: ``decode`` (``_decode`` alone, output_type "np": what a call without overlay pays)
and ``post`` (``_decode_overlay``).  The JSON holds every repeat, median, min and max per arm; the outputs of the two arms are compared
byte for byte.  Only the VAE is built: the back end runs no UNet."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def summary(xs):
    return dict(median_ms=round(1e3 * statistics.median(xs), 3), min_ms=round(1e3 * min(xs), 3), max_ms=round(1e3 * max(xs), 3),
                all_ms=[round(1e3 * x, 3) for x in xs])


def feathered_mask(rng, h=1024, w=768):
    """a torso-sized rectangle (jittered per request) whose edge ramps from 0 to 255 over 24 pixels"""
    t, l = 250 + int(rng.integers(-20, 21)), 150 + int(rng.integers(-20, 21))
    b, r = t + 550, l + 470
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    d = np.minimum(np.minimum(y - t, b - 1 - y), np.minimum(x - l, r - 1 - x))          # distance to the rectangle's edge, inside > 0
    return np.clip((d + 12) * 255 // 24, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", default="1,4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--pad", type=int, default=32)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_overlay_bench.json"))
    args = ap.parse_args()
    from PIL import Image
    from imagdressing_amd import ops
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet_inpainting as M
    from imagdressing_amd.vae import AutoencoderKL
    dev = torch.device("cuda", 0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    engine = types.SimpleNamespace(device=dev, dtype=dtype)          # (the back end asks the UNet for its device and type only)
    pipe = M.IMAGDressing_v1(vae=AutoencoderKL.random_init(seed=5, device=dev, dtype=dtype), reference_unet=engine, unet=engine, tokenizer=None,
                             text_encoder=None, controlnet=engine, image_encoder=None, ImgProj=None, scheduler=None)
    rng = np.random.default_rng(11)
    result = dict(tool="inpaint_overlay_bench", device=torch.cuda.get_device_name(dev), dtype=args.dtype, width=args.width, height=args.height,
                  padding_mask_crop=args.pad, output_type="pil", source_image="768 x 1024 RGB",
                  arms=dict(host="default route (switch off): Pillow resize, paste, composite", device="enable_device_image_io: pack, resample, imd_image_overlay"),
                  repeats=args.repeats, runs={})
    for R in [int(v) for v in args.requests.split(",")]:
        photos = [Image.fromarray(rng.integers(0, 256, size=(1024, 768, 3), dtype=np.uint8)) for _ in range(R)]
        masks = [Image.fromarray(feathered_mask(rng)) for _ in range(R)]
        gen = torch.Generator().manual_seed(5)
        final = torch.randn(R, 4, args.height // 8, args.width // 8, generator=gen).to(dev)
        fronts = {}
        for arm in ("host", "device"):
            pipe.enable_device_image_io(arm == "device")
            fronts[arm] = M._InpaintImages(pipe, photos, masks, (args.height, args.width), args.pad, dev)
            if arm == "device":
                for j in range(R):
                    fronts[arm].uploaded("image", j), fronts[arm].uploaded("mask_l", j)
        boxes = fronts["host"].boxes

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        times = {arm: dict(decode=[], post=[]) for arm in ("host", "device")}
        outs = {}
        for rep in range(args.repeats + 1):                      # repeat 0 warms both arms up and is dropped
            for arm in (("host", "device") if rep % 2 == 0 else ("device", "host")):
                pipe.enable_device_image_io(arm == "device")
                t_dec, _ = timed(lambda: pipe._decode(final, "np").images)
                t_post, img = timed(lambda: pipe._decode_overlay(final, "pil", fronts[arm]).images)
                outs[arm] = img
                if rep:
                    times[arm]["decode"].append(t_dec)
                    times[arm]["post"].append(t_post)
        pipe.disable_device_image_io()
        same = all(a.size == (768, 1024) and a.tobytes() == b.tobytes() for a, b in zip(outs["host"], outs["device"]))
        run = {arm: {k: summary(v) for k, v in times[arm].items()} for arm in times}
        run["boxes"] = [list(b) for b in boxes]
        run["box_share_of_photo"] = round(float(np.mean([(b[2] - b[0]) * (b[3] - b[1]) for b in boxes])) / (768 * 1024), 3)
        run["bit_identical"] = bool(same)
        run["post_median_speedup"] = round(run["host"]["post"]["median_ms"] / run["device"]["post"]["median_ms"], 4)
        run["image_io_launches_per_device_post"] = "1 pack, R resamples, R overlays"
        result["runs"][f"R{R}"] = run
        print(f"R={R}: " + json.dumps({arm: {k: run[arm][k]["median_ms"] for k in ("decode", "post")} for arm in ("host", "device")})
              + f" identical={same} boxes={run['boxes']}", flush=True)
    ops.clear_workspaces()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(tool="inpaint_overlay_bench", out=os.path.relpath(args.out, ROOT),
                          post_median_speedup={k: v["post_median_speedup"] for k, v in result["runs"].items()})), flush=True)


if __name__ == "__main__":
    main()
