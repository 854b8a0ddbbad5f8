"""The VAE mid block's attention as one flash launch (imd_attention at head dim 512; `AutoencoderKL.enable_flash_attention()`), and the sizes past
the 16384 tokens the three-launch route takes, where it runs whatever the switch says.  Bars: those of tests/test_vae_gpu.py (fp16 rms 0.5 %,
bf16 2.5 %), unchanged."""

import pytest
import torch
import torch.nn.functional as F

from tests.test_vae_gpu import bars, rnd, stats

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
MID512 = dict(block_out_channels=(64, 128, 256, 512), norm_num_groups=8)          # a small VAE whose mid block has the full 512 channels


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from imagdressing_amd import ops
    return ops


@pytest.fixture(scope="module")
def oracle(gpu):
    """The real 83.7 M-parameter VAE in fp32 on the CPU, computed once for both dtypes: weights, a 32x32 latent and its decode, a 128x128 image and
    its moments, the ragged 9x7 latent and its decode, a 10x6 latent."""
    from oracle import vae as OV
    sd = OV.seeded_state_dict(None, seed=3)
    o = OV.AutoencoderKL(); o.load_state_dict(sd, strict=True)
    z = rnd(4, 1, 4, 32, 32)
    img = rnd(5, 1, 3, 128, 128).clamp(-1, 1)
    z63, z60 = rnd(6, 1, 4, 9, 7), rnd(8, 1, 4, 10, 6)
    with torch.no_grad():
        return dict(sd=sd, z=z, dec=o.decode(z), img=img, moments=o.encode_moments(img), z63=z63, dec63=o.decode(z63), z60=z60)


_engines = {}


def engine(oracle, dt):
    """The HIP VAE on the oracle's weights, one per element type for the whole file; every test leaves its switch off."""
    from imagdressing_amd.vae import AutoencoderKL
    if dt not in _engines:
        _engines[dt] = AutoencoderKL(oracle["sd"], None, "cuda", dt)
    e = _engines[dt]
    e.disable_flash_attention()
    return e


class count_attention:
    """`with count_attention(ops) as c`: c.calls = the (D, B, N) of every ops.attention call inside."""

    def __init__(self, ops):
        self.ops, self.calls = ops, []

    def __enter__(self):
        self.real = self.ops.attention

        def counted(*a, **kw):
            self.calls.append((kw["D"], kw["B"], kw["N"]))
            return self.real(*a, **kw)
        self.ops.attention = counted
        return self

    def __exit__(self, *exc):
        self.ops.attention = self.real
        return False


def meets(got, ref, dt, what):
    st, b = stats(got, ref), bars(dt)
    print(f"{what}: {st}")
    assert bool(torch.isfinite(got.float()).all()), what
    assert st["rel_rms"] < b["rel_rms"] and st["max_abs"] < b["max_rel"] * st["ref_std"], (what, st)
    return st


@DTS
@torch.no_grad()
def test_flash_route_vs_oracle(gpu, oracle, dt):
    """Full-width decode of a 32x32 latent and encode of a 128x128 image with the switch on: one head-dim-512 launch each, inside the bars."""
    e = engine(oracle, dt)
    e.enable_flash_attention()
    with count_attention(gpu) as c:
        got = e.decode(oracle["z"].cuda(), return_dict=False)[0]
        dist = e.encode(oracle["img"].cuda()).latent_dist
    e.disable_flash_attention()
    assert c.calls == [(512, 1, 1024), (512, 1, 256)], c.calls
    assert got.shape == (1, 3, 256, 256) and got.dtype == dt
    meets(got, oracle["dec"], dt, "decode, flash")
    mean_o, logvar_o = oracle["moments"]
    assert dist.mean.shape == mean_o.shape
    meets(dist.mean, mean_o, dt, "encode mean, flash")
    meets(dist.logvar, logvar_o, dt, "encode logvar, flash")


@DTS
@torch.no_grad()
def test_default_route_is_unchanged(gpu, oracle, dt):
    """Switch off: no imd_attention launch, the same bits run after run.  Switch on: another result, both inside the bars (so no further apart than
    the two bars together)."""
    e = engine(oracle, dt)
    z = oracle["z"].cuda()
    with count_attention(gpu) as c:
        default = e.decode(z, return_dict=False)[0]
        again = e.decode(z, return_dict=False)[0]
    assert c.calls == [], f"the default route launched imd_attention: {c.calls}"
    assert torch.equal(default, again)
    e.enable_flash_attention()
    flash = e.decode(z, return_dict=False)[0]
    e.disable_flash_attention()
    after = e.decode(z, return_dict=False)[0]
    assert torch.equal(default, after), "disable_flash_attention() does not restore the default route"
    meets(default, oracle["dec"], dt, "decode, default")
    meets(flash, oracle["dec"], dt, "decode, flash")
    print(f"flash against default: {stats(flash, default)}")


@DTS
@torch.no_grad()
def test_past_the_limit(gpu, oracle, dt):
    """16448 tokens (8 x 2056), switch off: more columns than imd_softmax_rows takes -- raised ImdError before there was a flash kernel.  Reference:
    the block restated in fp32 torch on the GPU, softmax over chunks of query rows."""
    e = engine(oracle, dt)
    attn = e.d_mid.attn
    Cc, Hh, Ww = 512, 8, 2056
    N = Hh * Ww
    x = rnd(7, 1, Hh, Ww, Cc).to(dt).cuda()
    with count_attention(gpu) as c:
        got = attn(x)
    assert c.calls == [(512, 1, N)] and got.shape == x.shape and got.dtype == dt
    sd = {k: oracle["sd"][f"decoder.mid_block.attentions.0.{k}"].cuda().float() for k in
          ("group_norm.weight", "group_norm.bias", "to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias", "to_out.0.weight", "to_out.0.bias")}
    xf = x.float()                                                                     # [1, H, W, C]
    h = F.group_norm(xf.permute(0, 3, 1, 2), 32, sd["group_norm.weight"], sd["group_norm.bias"], eps=1e-6).permute(0, 2, 3, 1).reshape(N, Cc)
    q, k, v = (F.linear(h, sd[f"to_{n}.weight"], sd[f"to_{n}.bias"]) for n in "qkv")
    o = torch.cat([torch.softmax(q[i:i + 2048] @ k.t() * Cc ** -0.5, dim=-1) @ v for i in range(0, N, 2048)])
    ref = F.linear(o, sd["to_out.0.weight"], sd["to_out.0.bias"]) + xf.view(N, Cc)
    meets(got.view(N, Cc), ref, dt, "mid attention at 16448 tokens")


@DTS
@torch.no_grad()
def test_ragged_token_count(gpu, oracle, dt):
    """Token counts that are no multiple of the 32-key tile and less than one 64-key unit.
    A 9 x 7 latent, 63 tokens: the three launches cannot take it (their S = Q K^T GEMM needs a token count that is a multiple of 4), so there is
    no switch-off result to compare with; the switch-on decode is held to the bars against the fp32 oracle instead.
    A 10 x 6 latent, 60 tokens: switch on against switch off, each taken as the other's reference."""
    e = engine(oracle, dt)
    e.enable_flash_attention()
    with count_attention(gpu) as c:
        on63 = e.decode(oracle["z63"].cuda(), return_dict=False)[0]
        on60 = e.decode(oracle["z60"].cuda(), return_dict=False)[0]
    e.disable_flash_attention()
    assert c.calls == [(512, 1, 63), (512, 1, 60)] and on63.shape == (1, 3, 72, 56) and on60.shape == (1, 3, 80, 48)
    meets(on63, oracle["dec63"], dt, "63 tokens, flash against the fp32 oracle")
    off60 = e.decode(oracle["z60"].cuda(), return_dict=False)[0]
    meets(on60, off60.float(), dt, "60 tokens, flash against default")
    meets(off60, on60.float(), dt, "60 tokens, default against flash")


@torch.no_grad()
def test_pipeline_with_flash_vae(gpu):
    """`pipe.vae.enable_flash_attention()` is the surface: garment encode and decode of a 128x128 call run the head-dim-512 launch."""
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    from imagdressing_amd.scheduler import DDIMScheduler
    from imagdressing_amd.vae import AutoencoderKL
    from tests.harness import SMALL as USMALL, build_pair
    dt = torch.float16
    p = build_pair(USMALL, seed=0, dtype=dt)
    vae = AutoencoderKL.random_init(seed=5, config=MID512, device="cuda", dtype=dt)
    sch = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                        clip_sample=False, set_alpha_to_one=False, steps_offset=1)

    class Proj:
        def __call__(self, h):
            return h
    pipe = IMAGDressing_v1(vae=vae, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None,
                           image_encoder=None, ImgProj=Proj(), scheduler=sch, safety_checker=None, feature_extractor=None)
    pipe.vae.enable_flash_attention()
    garment = rnd(10, 1, 3, 128, 128).clamp(-1, 1).cuda()
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, width=128, height=128, num_inference_steps=2,
              guidance_scale=7.5, num_images_per_prompt=2, prompt_embeds=rnd(11, 1, 77, 64, scale=0.5).cuda(),
              negative_prompt_embeds=rnd(12, 1, 77, 64, scale=0.5).cuda(), ref_clip_hidden_states=rnd(13, 1, 16, 64, scale=0.5).cuda(),
              latents=rnd(14, 2, 4, 16, 16).cuda())
    with count_attention(gpu) as c:
        out = pipe(ref_image=garment, output_type="pt", **kw).images
    d512 = [x for x in c.calls if x[0] == 512]
    assert d512 == [(512, 1, 256), (512, 2, 256)], d512          # garment encode, then ONE launch for the two decoded images
    assert out.shape == (2, 3, 128, 128) and torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
    out2 = pipe(ref_image=garment, output_type="pt", **kw).images
    assert torch.equal(out, out2)
