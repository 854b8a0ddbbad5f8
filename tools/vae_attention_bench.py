"""The VAE mid block's attention on its two routes, on one MI355X: the default three launches per image (S = Q K^T, imd_softmax_rows, O = P V --
the yardstick) against the one flash launch at head dim 512 (`AutoencoderKL.enable_flash_attention()`), for the mid attention alone and for a
whole `decode`, at latents 64x64, 64x80, 96x128 and 128x128, B = 1 and 4, fp16 and bf16.  The two routes are timed in the same process,
interleaved: five repeats each of a window of device-event-timed calls, reported as median [min - max] in milliseconds per call.  Also the flash
route alone at 128x160 (20480 tokens: the three launches refuse it) and `torch.cuda.memory_allocated` after each route at 128x128.

    python tools/vae_attention_bench.py [--out profiles/vae_attention_bench.json]

Needs a GPU; writes the JSON and prints the table of the README."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from imagdressing_amd import ops
from imagdressing_amd.vae import AutoencoderKL, mid_attention_route

LATENTS = ((64, 64), (64, 80), (96, 128), (128, 128))
PAST = (128, 160)
BATCHES = (1, 4)
DTYPES = (("fp16", torch.float16), ("bf16", torch.bfloat16))
WINDOW_MS = 150.0          # a timed window holds at least this much work (and at least 2, at most 100 calls)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(arms, repeats):
    """arms: {name: fn}.  Warm every arm up, size its window, then `repeats` rounds that visit the arms in turn.  -> {name: dict(median, min, max, iters)}"""
    iters = {}
    for name, fn in arms.items():
        fn(); fn()
        torch.cuda.synchronize()
        one = window(fn, 2)
        iters[name] = max(2, min(100, int(WINDOW_MS / max(one, 1e-3)) + 1))
    times = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            times[name].append(window(fn, iters[name]))
    return {name: dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), iters=iters[name]) for name, t in times.items()}


def set_route(vae, flash):
    vae.enable_flash_attention(flash)


def measure(vae, dt, h, w, B, repeats, routes):
    N = h * w
    g = torch.Generator(device="cuda").manual_seed(h * 1000 + w + B)
    x = torch.randn(B, h, w, 512, generator=g, device="cuda").to(dt)
    z = torch.randn(B, 4, h, w, generator=g, device="cuda")
    attn = vae.d_mid.attn

    def arm(fn, flash):
        def run():
            set_route(vae, flash)
            return fn()
        return run
    row = dict(latent=f"{h}x{w}", tokens=N, B=B, attention_gflop=round(4.0 * B * N * N * 512 / 1e9, 1))
    for what, fn in (("attention", lambda: attn(x)), ("decode", lambda: vae.decode(z, return_dict=False)[0])):
        arms = {r: arm(fn, r == "flash") for r in routes}
        for r in routes:
            assert mid_attention_route(N, 512, r == "flash") == r, (N, r)
        try:
            row[what] = interleaved(arms, repeats)
        except ops.L.ImdError as e:          # (a size some other kernel of the call refuses is reported, not hidden)
            torch.cuda.synchronize()
            row[what] = {r: dict(error=str(e)) for r in routes}
    set_route(vae, False)
    return row


def memory(vae, dt, h, w):
    """bytes torch holds after one mid attention at B = 1 on each route, beyond the weights and the input: what stays (ops.workspace never frees)
    and the peak inside the call"""
    x = torch.randn(1, h, w, 512, device="cuda").to(dt)
    out = {}
    for route in ("gemm", "flash"):
        ops.clear_workspaces()
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        set_route(vae, route == "flash")
        y = vae.d_mid.attn(x)
        torch.cuda.synchronize()
        del y
        out[route] = dict(kept_bytes=torch.cuda.memory_allocated() - base, peak_bytes=torch.cuda.max_memory_allocated() - base)
    set_route(vae, False)
    ops.clear_workspaces()
    torch.cuda.empty_cache()
    return out


def fmt(t):
    if "error" in t:
        return "refused"
    return f"{t['median_ms']:.3f} [{t['min_ms']:.3f} - {t['max_ms']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vae_attention_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_attention_bench: needs a GPU (there is nothing to time without one)")
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=a.repeats, window_ms=WINDOW_MS,
               unit="milliseconds per call, device events around a window of calls; median [min - max] over the repeats, routes interleaved",
               both_routes={}, flash_only={}, memory_128x128={})
    for dname, dt in DTYPES:
        vae = AutoencoderKL.random_init(seed=5, device="cuda", dtype=dt)
        rows = []
        for h, w in LATENTS:
            for B in BATCHES:
                rows.append(measure(vae, dt, h, w, B, a.repeats, ("gemm", "flash")))
                print(dname, json.dumps(rows[-1]), flush=True)
                ops.clear_workspaces(); torch.cuda.empty_cache()
        res["both_routes"][dname] = rows
        res["flash_only"][dname] = [measure(vae, dt, PAST[0], PAST[1], B, a.repeats, ("flash",)) for B in BATCHES]
        print(dname, json.dumps(res["flash_only"][dname]), flush=True)
        res["memory_128x128"][dname] = memory(vae, dt, 128, 128)
        del vae
        ops.clear_workspaces(); torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("\n| latent | B | type | attention, three launches | attention, flash | decode, three launches | decode, flash |\n|---|---|---|---|---|---|---|")
    for dname, _ in DTYPES:
        for r in res["both_routes"][dname]:
            print(f"| {r['latent']} | {r['B']} | {dname} | {fmt(r['attention']['gemm'])} | {fmt(r['attention']['flash'])} | {fmt(r['decode']['gemm'])} | {fmt(r['decode']['flash'])} |")
        for r in res["flash_only"][dname]:
            print(f"| {r['latent']} | {r['B']} | {dname} | refused | {fmt(r['attention']['flash'])} | refused | {fmt(r['decode']['flash'])} |")
    for dname, _ in DTYPES:
        m = res["memory_128x128"][dname]
        print(f"memory at 128x128, B = 1, {dname}: three launches keep {m['gemm']['kept_bytes'] / 2 ** 20:.0f} MiB (peak {m['gemm']['peak_bytes'] / 2 ** 20:.0f} MiB), "
              f"flash keeps {m['flash']['kept_bytes'] / 2 ** 20:.0f} MiB (peak {m['flash']['peak_bytes'] / 2 ** 20:.0f} MiB)")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
