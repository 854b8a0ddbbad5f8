"""What ``mask_dilate`` / ``mask_blur`` of an inpainting call cost, host route (Pillow) against device route (``imd_image_mask_filter``).

    python tools/mask_filter_bench.py [--requests 1,4] [--blurs 4,16,33] [--dilate 8] [--repeats 5] [--out profiles/mask_filter_bench.json]

Workload: hard-edged human-parsing-like masks of 768 x 1024 (a torso rectangle, jittered per request) beside 768 x 1024 photos, grown by
``mask_dilate`` = 8 and feathered with ``mask_blur`` = 4 / 16 / 33, for R = 1 and R = 4 requests, ``padding_mask_crop`` = 32 at 512 x 640.

Two arms, interleaved repeat by repeat in ONE process on one device (arm order alternates), the protocol of tools/image_io_bench.py:
  host    the default route: per mask ``convert("L").filter(MaxFilter(17)).filter(GaussianBlur(b))`` on one host thread, then the front
          end through Pillow
  device  ``enable_device_image_io()``: the uploaded mask through ``imd_image_mask_filter`` (three launches and one for the bounds), the
          crop box from ONE read-back of the bounds, then the front end on the device
Times are host wall time between device-wide syncs: ``filter`` (the filter alone -- host: the Pillow calls on the "L" masks; device:
the launches on masks that are uploaded already, with the read-back of the bounds), ``blur_only`` (the same with ``mask_dilate`` = 0:
Pillow's MaxFilter is a rank filter over the whole window and dominates the host arm) and ``front`` (the whole front end of the call: filter,
crop boxes, person-image windows, binarised latent masks and the built-in inpaint condition, uploads included).  The JSON holds every
repeat, median, min and max per arm; the filtered masks, boxes and front-end tensors of the two arms are compared bit for bit.  No engine
is built: the front end runs no network."""
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


def hard_mask(rng, h=1024, w=768):
    t, l = 250 + int(rng.integers(-20, 21)), 150 + int(rng.integers(-20, 21))
    m = np.zeros((h, w), np.uint8)
    m[t:t + 550, l:l + 470] = 255
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", default="1,4")
    ap.add_argument("--blurs", default="4,16,33")
    ap.add_argument("--dilate", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--pad", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_filter_bench.json"))
    args = ap.parse_args()
    import PIL
    from PIL import Image
    from imagdressing_amd import ops
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet_inpainting as M
    from imagdressing_amd.image import mask_filter_host
    dev = torch.device("cuda", 0)
    engine = types.SimpleNamespace(device=dev, dtype=torch.float16)          # (the front end asks the UNet for its device and type only)
    pipe = M.IMAGDressing_v1(vae=None, reference_unet=engine, unet=engine, tokenizer=None, text_encoder=None, controlnet=engine,
                             image_encoder=None, ImgProj=None, scheduler=None)
    size, k = (args.height, args.width), args.dilate
    rng = np.random.default_rng(11)
    result = dict(tool="mask_filter_bench", device=torch.cuda.get_device_name(dev), pillow=PIL.__version__, mask="768 x 1024 L, hard-edged",
                  mask_dilate=k, width=args.width, height=args.height, padding_mask_crop=args.pad,
                  arms=dict(host="default route: Pillow MaxFilter + GaussianBlur, Pillow front end",
                            device="enable_device_image_io: imd_image_mask_filter, device front end"),
                  repeats=args.repeats, runs={})

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for R in [int(v) for v in args.requests.split(",")]:
        photos = [Image.fromarray(rng.integers(0, 256, size=(1024, 768, 3), dtype=np.uint8)) for _ in range(R)]
        masks = [Image.fromarray(hard_mask(rng)) for _ in range(R)]
        pipe.enable_device_image_io()
        proc = pipe._image_processor()
        ups = [proc._upload(m, "L") for m in masks]
        for b in [float(v) for v in args.blurs.split(",")]:
            def filter_alone(arm, k=k):
                if arm == "host":
                    return [mask_filter_host(m, k, b) for m in masks]
                res = [proc.mask_filter(u, k, b, bounds=True) for u in ups]
                return [r[0] for r in res], torch.cat([r[1] for r in res]).cpu().tolist()

            def front_end(arm):
                if arm == "host":
                    front = M._InpaintImages(pipe, photos, [mask_filter_host(m, k, b) for m in masks], size, args.pad, dev)
                else:
                    front = M._InpaintImages(pipe, photos, masks, size, args.pad, dev, mask_filter=[(k, b)] * R)
                return front, front.image_tensor(8), front.mask_latents(size[0] // 8, size[1] // 8), front.control(None, 8)

            times = {arm: dict(filter=[], blur_only=[], front=[]) for arm in ("host", "device")}
            outs = {}
            for rep in range(args.repeats + 1):                      # repeat 0 warms both arms up and is dropped
                for arm in (("host", "device") if rep % 2 == 0 else ("device", "host")):
                    pipe.enable_device_image_io(arm == "device")
                    t_f, filt = timed(lambda: filter_alone(arm))
                    t_b, _ = timed(lambda: filter_alone(arm, 0))     # (the Gaussian without the window maximum: where the host time goes)
                    t_e, fe = timed(lambda: front_end(arm))
                    outs[arm] = (filt, fe)
                    if rep:
                        times[arm]["filter"].append(t_f)
                        times[arm]["blur_only"].append(t_b)
                        times[arm]["front"].append(t_e)
            host_masks, (dev_masks, _) = outs["host"][0], outs["device"][0]
            fh, fd = outs["host"][1], outs["device"][1]
            same = all(torch.equal(torch.from_numpy(np.array(hm)), dm[0, ..., 0].cpu()) for hm, dm in zip(host_masks, dev_masks))
            same = same and fh[0].boxes == fd[0].boxes and torch.equal(fh[1].cpu(), fd[1].cpu()) and torch.equal(fh[2].cpu(), fd[2].cpu())
            run = {arm: {key: summary(v) for key, v in times[arm].items()} for arm in times}
            run["boxes"] = [list(bx) for bx in fh[0].boxes]
            run["bit_identical"] = bool(same)
            for key in ("filter", "blur_only", "front"):
                run[key + "_median_speedup"] = round(run["host"][key]["median_ms"] / run["device"][key]["median_ms"], 4)
            result["runs"][f"R{R}_blur{b:g}"] = run
            print(f"R={R} blur={b:g}: " + json.dumps({arm: {key: run[arm][key]["median_ms"] for key in ("filter", "blur_only", "front")} for arm in ("host", "device")})
                  + f" identical={same}", flush=True)
    pipe.disable_device_image_io()
    ops.clear_workspaces()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh_:
        json.dump(result, fh_, indent=1)
        fh_.write("\n")
    print(json.dumps(dict(tool="mask_filter_bench", out=os.path.relpath(args.out, ROOT),
                          filter_median_speedup={key: v["filter_median_speedup"] for key, v in result["runs"].items()},
                          front_median_speedup={key: v["front_median_speedup"] for key, v in result["runs"].items()})), flush=True)


if __name__ == "__main__":
    main()
