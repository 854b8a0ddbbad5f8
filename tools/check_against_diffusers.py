#!/usr/bin/env python
"""Pin the UNPINNED oracles against the library they restate -- the one route from "parity unpinned" to "green".

    python tools/check_against_diffusers.py [--full]

``oracle/sd15.py`` (UNet2DConditionModel, ControlNetModel), ``oracle/vae.py`` (AutoencoderKL), ``oracle/ddim.py`` and
``oracle/unipc.py`` restate ``diffusers==0.24.0`` (/root/reference/requirements.txt:12), which is not vendored in the reference and
not installable offline -- nothing in this repository could check them against the library itself.  Where an environment HAS
diffusers 0.24.x, this script instantiates the library's own classes from config (no weights needed: the same seeded synthetic
state dicts the tests use are loaded into both sides, the key names are the library's), runs them on seeded inputs on the CPU in
fp32 and compares with the oracles to 1e-5 (models) / 1e-6 (schedulers, float64 where the library allows it).

Exit status: 0 = every comparison passed, OR diffusers is absent ("parity unpinned" stays the honest label); 1 = a comparison
failed (the oracle disagrees with the library: fix the oracle); 2 = diffusers present but not 0.24.x (results are printed, the
pin is not claimed).  ``--full`` also runs the full-width SD1.5 configuration (859.5 M parameters; a few minutes of CPU time)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the real library must win over the opt-in import shim in <repo>/compat
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.join(ROOT, "compat")]
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def find_diffusers():
    try:
        import diffusers
    except Exception as e:        # noqa: BLE001
        return None, f"import failed: {type(e).__name__}: {e}"
    ver = getattr(diffusers, "__version__", "?")
    if "imagdressing_amd" in ver or os.path.abspath(getattr(diffusers, "__file__", "")).startswith(os.path.join(ROOT, "compat")):
        return None, "only the repository's own import shim (<repo>/compat/diffusers) is on the path, not the library"
    return diffusers, ver


def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def report(name, got, ref, tol, results):
    err = (got.double() - ref.double()).abs().max().item()
    scale = max(ref.double().abs().max().item(), 1e-30)
    ok = err <= tol * max(1.0, scale)
    results.append((name, ok, err, scale))
    print(f"  {'ok  ' if ok else 'FAIL'} {name}: max abs diff {err:.3e} (ref max {scale:.3e}, bar {tol:.0e} x max(1, ref max))")


@torch.no_grad()
def check_unet(diffusers, cfg_small, results, label):
    from imagdressing_amd import unet as E
    from oracle import sd15
    from tests.harness import oracle_cfg
    full = dict(E.SD15_CONFIG, **cfg_small)
    sd = E.random_state_dict(E.unet_param_shapes(full), 0)
    lib = diffusers.UNet2DConditionModel(
        sample_size=64, in_channels=4, out_channels=4, layers_per_block=2, block_out_channels=tuple(full["block_out_channels"]),
        down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",), up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3,
        cross_attention_dim=full["cross_attention_dim"], attention_head_dim=full["attention_head_dim"], norm_num_groups=full["norm_num_groups"],
        use_linear_projection=False, flip_sin_to_cos=True, freq_shift=0)
    lib.load_state_dict(sd, strict=True)
    orc = sd15.UNet2DConditionModel(oracle_cfg(cfg_small))
    orc.load_state_dict(sd, strict=True)
    hw = 16 if cfg_small else 32
    x, ehs = rnd(1, 2, 4, hw, hw), rnd(2, 2, 77, full["cross_attention_dim"], scale=0.5)
    report(f"UNet2DConditionModel forward [{label}]", orc(x, 481, ehs), lib(x, 481, ehs).sample, 1e-5, results)
    # with ControlNet residuals
    sdc = E.random_state_dict(E.controlnet_param_shapes(full), 2, zero_convs=True)
    libc = diffusers.ControlNetModel(
        in_channels=4, layers_per_block=2, block_out_channels=tuple(full["block_out_channels"]),
        down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",), cross_attention_dim=full["cross_attention_dim"],
        attention_head_dim=full["attention_head_dim"], norm_num_groups=full["norm_num_groups"], use_linear_projection=False,
        conditioning_embedding_out_channels=(16, 32, 96, 256))
    libc.load_state_dict(sdc, strict=True)
    orcc = sd15.ControlNetModel(oracle_cfg(cfg_small))
    orcc.load_state_dict(sdc, strict=True)
    cond = torch.rand(2, 3, hw * 8, hw * 8, generator=torch.Generator().manual_seed(3))
    dl, ml = libc(x, 481, ehs, cond, conditioning_scale=0.9, return_dict=False)
    do, mo = orcc(x, 481, ehs, cond, 0.9)
    for i, (a, b) in enumerate(zip(do, dl)):
        report(f"ControlNetModel down residual {i} [{label}]", a, b, 1e-5, results)
    report(f"ControlNetModel mid residual [{label}]", mo, ml, 1e-5, results)
    report(f"UNet2DConditionModel + residuals [{label}]",
           orc(x, 481, ehs, down_block_additional_residuals=list(do), mid_block_additional_residual=mo),
           lib(x, 481, ehs, down_block_additional_residuals=tuple(dl), mid_block_additional_residual=ml).sample, 1e-5, results)


@torch.no_grad()
def check_vae(diffusers, results):
    from oracle import vae as OV
    cfg = dict(block_out_channels=(64, 128, 128, 128), norm_num_groups=8)
    sd = OV.seeded_state_dict(cfg, seed=0)
    lib = diffusers.AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 4,
                                  up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=cfg["block_out_channels"], layers_per_block=2,
                                  latent_channels=4, norm_num_groups=8)
    lib.load_state_dict(sd, strict=True)
    orc = OV.AutoencoderKL(cfg)
    orc.load_state_dict(sd, strict=True)
    img, z = rnd(4, 1, 3, 64, 64), rnd(5, 1, 4, 8, 8)
    report("AutoencoderKL.encode(...).latent_dist.mean", orc.encode_moments(img)[0], lib.encode(img).latent_dist.mean, 1e-5, results)
    report("AutoencoderKL.decode", orc.decode(z), lib.decode(z, return_dict=False)[0], 1e-5, results)


@torch.no_grad()
def check_schedulers(diffusers, results):
    from oracle.ddim import DDIMOracle
    from oracle.unipc import UniPCOracle
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    lib = diffusers.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kw)     # inference_IMAGdressing.py:119-127
    orc = DDIMOracle()
    for n in (20, 50):
        lib.set_timesteps(n)
        ts = orc.set_timesteps(n)
        report(f"DDIMScheduler.timesteps ({n} steps)", ts.double(), lib.timesteps.double(), 0.0, results)
        z = rnd(6, 1, 4, 8, 8).double()
        zl = z.clone()
        for i, t in enumerate(ts):
            eps = rnd(100 + i, 1, 4, 8, 8).double()
            z = orc.step(eps, t, z)
            zl = lib.step(eps, lib.timesteps[i], zl).prev_sample
        report(f"DDIMScheduler {n}-step trajectory", z, zl, 1e-6, results)
        noise, x0 = rnd(7, 1, 4, 8, 8), rnd(8, 1, 4, 8, 8)
        if hasattr(orc, "add_noise"):
            report(f"DDIMScheduler.add_noise (t = {int(ts[3])})", orc.add_noise(x0, noise, ts[3]), lib.add_noise(x0, noise, lib.timesteps[3:4]), 1e-6, results)
    libu = diffusers.UniPCMultistepScheduler(**kw)
    orcu = UniPCOracle()
    for n in (10, 50):
        libu.set_timesteps(n)
        ts = orcu.set_timesteps(n)
        report(f"UniPCMultistepScheduler.timesteps ({n} steps)", ts.double(), libu.timesteps.double(), 0.0, results)
        z = rnd(9, 1, 4, 8, 8).double()
        zl = z.clone()
        for i, t in enumerate(ts):
            eps = rnd(200 + i, 1, 4, 8, 8).double()
            z = orcu.step(eps, t, z)
            zl = libu.step(eps, libu.timesteps[i], zl).prev_sample
        report(f"UniPCMultistepScheduler {n}-step trajectory", z, zl, 1e-6, results)
    # the samplers on the fused step: tests/sampler_oracle.py (library-form restatements, what imagdressing_amd/scheduler.py is tested against).
    # The DPM-Solver++ restatement ends at sigma = 0, the 0.24 library at the sigma of training timestep 0: its last step is expected to differ.
    from tests import sampler_oracle as SO
    for cls, orc_cls, lib_kw, orc_kw in (
            ("DPMSolverMultistepScheduler", SO.DPMSolverOracle, {}, {}),
            ("DPMSolverMultistepScheduler", SO.DPMSolverOracle, dict(use_karras_sigmas=True), dict(use_karras_sigmas=True)),
            ("EulerDiscreteScheduler", SO.EulerOracle, {}, {}),
            ("EulerDiscreteScheduler", SO.EulerOracle, dict(timestep_spacing="leading", steps_offset=1), dict(timestep_spacing="leading", steps_offset=1)),
            ("EulerAncestralDiscreteScheduler", SO.EulerAncestralOracle, {}, {}),
            ("PNDMScheduler", SO.PNDMOracle, dict(skip_prk_steps=True, steps_offset=1), {})):
        libs = getattr(diffusers, cls)(**kw, **lib_kw)
        orcs = orc_cls(**orc_kw)
        tag = cls + (f" {lib_kw}" if lib_kw else "")
        for n in (10, 25):
            libs.set_timesteps(n)
            ts = orcs.set_timesteps(n)
            report(f"{tag}.timesteps ({n} steps)", ts.double(), libs.timesteps.double().cpu(), 1e-3, results)
            if hasattr(orcs, "sigmas") and hasattr(libs, "sigmas"):
                report(f"{tag}.sigmas ({n} steps, without the final one)", torch.as_tensor(orcs.sigmas[:-1]).double(), libs.sigmas[:-1].double().cpu(), 1e-6, results)
            if cls == "EulerAncestralDiscreteScheduler":
                continue          # the library draws the per-step noise itself: schedule and sigmas only (the step shares EulerOracle's arithmetic)
            z = rnd(9, 1, 4, 8, 8).double() * orcs.init_noise_sigma
            zl = z.clone()
            last = len(ts) - (1 if cls == "DPMSolverMultistepScheduler" else 0)
            for i, t in enumerate(ts[:last]):
                eps = rnd(300 + i, 1, 4, 8, 8).double()
                z = orcs.step(eps, t, z)
                zl = libs.step(eps, libs.timesteps[i], zl).prev_sample
            report(f"{tag} {n}-step trajectory" + (" (all but the last step)" if last < len(ts) else ""), z, zl, 1e-6, results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="also compare the full-width SD1.5 UNet / ControlNet (859.5 M / 361.3 M parameters)")
    a = ap.parse_args()
    diffusers, ver = find_diffusers()
    if diffusers is None:
        print(f"diffusers absent ({ver}) -- oracle/sd15.py, oracle/vae.py, oracle/ddim.py, oracle/unipc.py and tests/sampler_oracle.py stay UNPINNED "
              "(anchored on parameter counts, key names and schedule values only).  Install diffusers==0.24.0 to run this check.")
        return 0
    print(f"diffusers {ver} found at {os.path.dirname(diffusers.__file__)}")
    pinned = ver.startswith("0.24.")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    results = []
    from tests.harness import SMALL
    check_unet(diffusers, SMALL, results, "reduced width")
    if a.full:
        check_unet(diffusers, {}, results, "SD1.5 full width")
    check_vae(diffusers, results)
    check_schedulers(diffusers, results)
    bad = [r for r in results if not r[1]]
    print(f"{len(results) - len(bad)} / {len(results)} comparisons passed")
    if bad:
        return 1
    if not pinned:
        print(f"NOTE: diffusers {ver} is not 0.24.x (the reference's pin, requirements.txt:12): agreement is reported, the pin is not claimed")
        return 2
    print("oracles PINNED against diffusers " + ver)
    return 0


if __name__ == "__main__":
    sys.exit(main())
