"""enable_device_noise through the pipelines (SMALL config, 16 x 16 latents).  Switch off: the call is the call of before -- the same
launches per entry point, the bits of torch's draws, no imd_noise_rows launch.  Switch on: a seed is a reproducible stream per request,
Euler-ancestral replays under enable_step_graph bit for bit, and the final latents equal the switch-off loop fed the ORACLE's noise
through ``latents=`` / ``noise=`` / ``variance_noise=`` within the bars the same pipelines meet against their oracles
(test_e2e_gpu._traj_bar) -- Euler-ancestral, DDIM with eta = 0.5, and the inpainting blend with strength < 1."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import device_noise_oracle as O  # noqa: E402
from tests.harness import SMALL, build_pair, err_stats  # noqa: E402
from tests.test_e2e_gpu import _traj_bar  # noqa: E402
from tests.test_guidance_rescale_pipeline_gpu import _inpaint_kw, _kw, _pipe  # noqa: E402
from tests.test_multi_request_gpu import _Requests  # noqa: E402
from tests.unipc_cases import KW  # noqa: E402

STEPS, SEED = 6, 0x0123456789ABCDEF


def _sched(name):
    from imagdressing_amd import scheduler as S
    return {"ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **KW),
            "euler_a": lambda: S.EulerAncestralDiscreteScheduler(**KW), "dpm": lambda: S.DPMSolverMultistepScheduler(**KW)}[name]()


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def pair(request):
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=5, with_controlnet=True, dtype=request.param)
    p["dtype"] = request.param
    return p


def _call_kw(steps=STEPS, **over):
    kw = _kw(steps=steps)
    kw.pop("latents")
    kw.update(over)
    return kw


def _draw(seed, image, draw, h=16, w=16):
    """the oracle's draw as the [1, 4, h, w] fp32 tensor a caller would pass"""
    return torch.from_numpy(O.nchw(O.normals(seed, image, draw, h * w), h, w)).float()


class _Counting:
    """the loaded library with every call counted by entry point"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _counted_call(monkeypatch, pipe, **kw):
    from imagdressing_amd import _lib
    proxy = _Counting(_lib.load())
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", lambda: proxy)
        out = pipe(**kw).images
    # launches only: the dispatcher's pure queries are asked once per shape and then answered from its decision cache
    pure = ("_supported", "_auto_split", "_auto_cfg", "_parts", "_form", "_workspace_floats", "_padded_dims", "_tuning", "_version", "_error", "_check")
    return out, {k: v for k, v in proxy.calls.items() if not k.endswith(pure)}


@pytest.mark.parametrize("name", ["euler_a", "ddim"])
@torch.no_grad()
def test_switch_off_is_the_call_of_before(pair, monkeypatch, name):
    from imagdressing_amd import ops
    from imagdressing_amd.dressing_sd.pipelines._base import randn_tensor
    eta = 0.5 if name == "ddim" else 0.0
    pipe = _pipe(pair, _sched(name))
    before = ops.NOISE_COUNTER["launches"]
    gen = lambda: torch.Generator("cuda").manual_seed(5)          # noqa: E731
    fresh, calls = _counted_call(monkeypatch, pipe, **_call_kw(generator=gen(), eta=eta))
    # what the switch-off loop draws, by hand: the initial latents in fp32, then one draw per step in the UNet's element type
    G = gen()
    lat = randn_tensor((1, 4, 16, 16), generator=G, device=torch.device("cuda"), dtype=torch.float32)
    vn = [randn_tensor((1, 4, 16, 16), generator=G, device=torch.device("cuda"), dtype=pair["dtype"]) for _ in range(STEPS)]
    assert torch.isfinite(fresh).all() and torch.equal(pipe(**_call_kw(latents=lat, variance_noise=vn, eta=eta)).images, fresh)
    assert pipe.enable_device_noise() is pipe and pipe.disable_device_noise() is pipe
    again, calls2 = _counted_call(monkeypatch, pipe, **_call_kw(generator=gen(), eta=eta))
    assert torch.equal(again, fresh) and calls2 == calls
    assert "imd_noise_rows" not in calls and ops.NOISE_COUNTER["launches"] == before
    assert calls["imd_ddim_cfg_step" if name == "ddim" else "imd_sampler_step"] == STEPS
    with pytest.raises(ValueError, match=r"enable_device_noise\(\)"):
        pipe(seed=3, **_call_kw())
    assert not hasattr(pipe, "last_seeds")


@torch.no_grad()
def test_a_seed_is_a_reproducible_stream(pair, monkeypatch):
    pipe = _pipe(pair, _sched("euler_a")).enable_device_noise()
    a, calls = _counted_call(monkeypatch, pipe, seed=SEED, **_call_kw())
    assert pipe.last_seeds == [SEED]
    assert calls["imd_noise_rows"] == 1 + STEPS and calls["imd_sampler_step"] == STEPS          # draw 0, then one launch per step
    assert torch.isfinite(a).all() and torch.equal(pipe(seed=SEED, **_call_kw()).images, a)
    assert not torch.equal(pipe(seed=SEED + 1, **_call_kw()).images, a)
    assert not torch.equal(pipe(seed=SEED ^ (1 << 63), **_call_kw()).images, a)                  # the high word counts
    # generator -> its initial seed; no seed at all -> os.urandom, left in last_seeds
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(SEED), **_call_kw()).images, a) and pipe.last_seeds == [SEED]
    b = pipe(**_call_kw()).images
    assert len(pipe.last_seeds) == 1 and torch.equal(pipe(seed=pipe.last_seeds[0], **_call_kw()).images, b)
    # latents= / variance_noise= still win: given both, nothing is drawn
    vn = [_draw(SEED, 0, 1 + i).cuda() for i in range(STEPS)]
    _, calls = _counted_call(monkeypatch, pipe, seed=SEED, latents=_draw(SEED, 0, 0).cuda(), variance_noise=vn, **_call_kw())
    assert "imd_noise_rows" not in calls
    _, calls = _counted_call(monkeypatch, pipe, seed=SEED, variance_noise=vn, **_call_kw())
    assert calls["imd_noise_rows"] == 1
    with pytest.raises(ValueError, match="seed"):
        pipe(seed=-1, **_call_kw())
    with pytest.raises(ValueError, match="seed"):
        pipe(seed=[1, 2], **_call_kw())


@torch.no_grad()
def test_seed_lists_give_one_stream_per_request_and_images_differ(pair):
    pipe = _pipe(pair, _sched("euler_a")).enable_device_noise()
    reqs = _Requests(R=2)
    kw = dict(reqs.call_kwargs(guidance=(5.0, 7.0), image_scale=(1.0, 1.0)), num_inference_steps=4)
    kw.pop("latents")
    ab = pipe(seed=[11, 22], **kw).images
    assert pipe.last_seeds == [11, 22] and ab.shape[0] == 2 and torch.isfinite(ab).all()
    ac = pipe(seed=[11, 33], **kw).images
    assert torch.equal(ab[0], ac[0]) and not torch.equal(ab[1], ac[1])
    assert torch.equal(pipe(seed=[11, 22], **kw).images, ab)
    with pytest.raises(ValueError, match="2 requests"):
        pipe(seed=[1, 2, 3], **kw)
    # two images of one request: counter word image = 0, 1 -- different noise
    two = pipe(seed=SEED, **_call_kw(num_images_per_prompt=2, steps=3)).images
    assert two.shape[0] == 2 and not torch.equal(two[0], two[1])


@torch.no_grad()
def test_euler_ancestral_replays_under_step_graph(pair):
    pipe = _pipe(pair, _sched("euler_a")).enable_device_noise()
    reqs = _Requests(R=2)
    kw = dict(reqs.call_kwargs(guidance=(5.0, 7.0), image_scale=(1.0, 1.0)), num_inference_steps=6, seed=[5, 2 ** 64 - 1])
    kw.pop("latents")
    eager = pipe(**kw).images
    assert getattr(pipe, "_last_step_graph", None) is None
    pipe.enable_step_graph(True)
    try:
        g1 = pipe(**kw).images
        assert getattr(pipe, "_last_step_graph", None) is not None          # the graph path really ran
        g2 = pipe(**kw).images
    finally:
        pipe.enable_step_graph(False)
    assert torch.isfinite(eager).all() and torch.equal(eager, g1) and torch.equal(eager, g2)


def _close(p, got, ref, what):
    st = err_stats(got, ref)
    bar = _traj_bar(p["dtype"])
    print(f"device noise vs the host loop fed the oracle's noise, {what}[{p['dtype']}]: {st}")
    assert torch.isfinite(got).all()
    assert st["max_abs"] < bar["max_abs"] * max(st["ref_std"], 1.0) and st["rel_rms"] < bar["rel_rms"], (what, st)


@pytest.mark.parametrize("name", ["euler_a", "ddim"])
@torch.no_grad()
def test_final_latents_equal_the_host_loop_fed_the_oracles_noise(pair, name):
    """draw 0 through ``latents=``, draw 1 + i through ``variance_noise=[i]`` into the SWITCH-OFF call"""
    eta = 0.5 if name == "ddim" else 0.0
    off = _pipe(pair, _sched(name))
    ref = off(latents=_draw(SEED, 0, 0).cuda(), variance_noise=[_draw(SEED, 0, 1 + i).cuda() for i in range(STEPS)], **_call_kw(eta=eta)).images
    on = _pipe(pair, _sched(name)).enable_device_noise()
    got = on(seed=SEED, **_call_kw(eta=eta)).images
    _close(pair, got, ref, name)
    other = on(seed=SEED + 1, **_call_kw(eta=eta)).images
    assert err_stats(other, ref)["rel_rms"] > 10 * _traj_bar(pair["dtype"])["rel_rms"]          # the seed is no rounding-level change
    if name == "ddim":          # eta = 0: no per-step noise, only draw 0
        assert torch.equal(on(seed=SEED, **_call_kw()).images, on(seed=SEED, **_call_kw(eta=0.0)).images)


@pytest.mark.parametrize("name", ["euler_a", "ddim"])
@torch.no_grad()
def test_inpainting_blend_with_strength(pair, name):
    """strength 0.6 of 10 steps: t_start = 4, so the steps read draws 5 .. 10; draw 0 is add_noise's noise AND the blend's"""
    steps, strength = 10, 0.6
    eta = 0.5 if name == "ddim" else 0.0
    kw, mask, img_lat = _inpaint_kw(steps, strength)
    kw.pop("noise")
    t_start, run = 4, 6
    off = _pipe(pair, _sched(name), "inpainting")
    ref = off(noise=_draw(SEED, 0, 0, 16, 24).cuda(), variance_noise=[_draw(SEED, 0, 1 + t_start + i, 16, 24).cuda() for i in range(run)], eta=eta, **kw).images
    on = _pipe(pair, _sched(name), "inpainting").enable_device_noise()
    got = on(seed=SEED, eta=eta, **kw).images
    _close(pair, got, ref, f"inpainting {name}")
    keep = (mask == 0).expand(1, 4, -1, -1)
    assert torch.equal(got.cpu()[keep], img_lat[keep])                       # outside the mask the final latent IS the image latent
    assert torch.equal(on(seed=SEED, eta=eta, **kw).images, got)
    # shifted draws would not pass: the numbering is the absolute one
    wrong = off(noise=_draw(SEED, 0, 0, 16, 24).cuda(), variance_noise=[_draw(SEED, 0, 1 + i, 16, 24).cuda() for i in range(run)], eta=eta, **kw).images
    assert err_stats(wrong, ref)["rel_rms"] > 10 * _traj_bar(pair["dtype"])["rel_rms"]
