"""Request-batched pipeline calls without a GPU: argument validation of all four pipelines, the row <-> request / prompt / garment
layout, and the C entry point of the per-row fused DDIM step (declared, bound, exported, size-checked)."""
import ctypes
import os
import re

import pytest
import torch

from imagdressing_amd.dressing_sd.pipelines._base import RequestLayout, per_call_value, per_request_floats, request_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub:
    """stands in for the engine UNets: validation must refuse a bad call before any model is touched"""
    device = torch.device("cpu")
    dtype = torch.float16

    @property
    def attn_processors(self):
        raise AssertionError("the call reached the model")

    def forward_nhwc(self, *a, **k):
        raise AssertionError("the call reached the model")


def _sched(unipc=False):
    from imagdressing_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
    cls = UniPCMultistepScheduler if unipc else DDIMScheduler
    return cls(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
               set_alpha_to_one=False, steps_offset=1)


def _pipe(kind, unipc=False):
    from imagdressing_amd.dressing_sd.pipelines import (IMAGDressing_v1_pipeline, IMAGDressing_v1_pipeline_controlnet,
                                                        IMAGDressing_v1_pipeline_controlnet_inpainting, IMAGDressing_v1_pipeline_ipa_controlnet)
    common = dict(vae=None, reference_unet=_Stub(), unet=_Stub(), tokenizer=None, text_encoder=None, image_encoder=None,
                  ImgProj=lambda h: h, scheduler=_sched(unipc))
    if kind == "base":
        return IMAGDressing_v1_pipeline.IMAGDressing_v1(**common)
    if kind == "controlnet":
        return IMAGDressing_v1_pipeline_controlnet.IMAGDressing_v1(controlnet=_Stub(), **common)
    if kind == "inpaint":
        return IMAGDressing_v1_pipeline_controlnet_inpainting.IMAGDressing_v1(controlnet=_Stub(), **common)
    pipe = IMAGDressing_v1_pipeline_ipa_controlnet.IMAGDressing_v1.__new__(IMAGDressing_v1_pipeline_ipa_controlnet.IMAGDressing_v1)
    pipe._init_common(controlnet=_Stub(), **common)          # (no image_proj_model: nothing past validation may run)
    return pipe


def _kw(R=3, **over):
    kw = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=4,
              guidance_scale=7.5, prompt_embeds=torch.zeros(R, 77, 64), negative_prompt_embeds=torch.zeros(R, 77, 64),
              ref_clip_hidden_states=torch.zeros(R, 16, 64), ref_image_latents=torch.zeros(R, 4, 16, 16), output_type="latent")
    kw.update(over)
    return kw


KINDS = ["base", "controlnet", "inpaint", "ipa"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,value", [("ref_image_latents", torch.zeros(2, 4, 16, 16)), ("ref_clip_hidden_states", torch.zeros(2, 16, 64)),
                                        ("negative_prompt_embeds", torch.zeros(2, 77, 64)), ("guidance_scale", [5.0, 7.5]),
                                        ("image_scale", [1.0, 0.5])])
def test_length_mismatch_names_the_argument(kind, name, value):
    with pytest.raises(ValueError, match=name):
        _pipe(kind)(**_kw(**{name: value}))


@pytest.mark.parametrize("kind,name,value", [("base", "num_inference_steps", [4, 5, 4]), ("base", "eta", [0.0, 0.5, 0.0]),
                                             ("controlnet", "controlnet_conditioning_scale", [1.0, 0.5, 1.0]),
                                             ("inpaint", "strength", [1.0, 0.5, 1.0]), ("ipa", "ipa_scale", [0.9, 0.5, 0.9]),
                                             ("ipa", "s_lora_scale", [0.2, 0.1, 0.2]), ("ipa", "c_lora_scale", [0.2, 0.2, 0.1])])
def test_per_call_arguments_refuse_differing_sequences(kind, name, value):
    with pytest.raises(ValueError, match=name):
        _pipe(kind)(**_kw(**{name: value}))


def test_per_call_value_accepts_equal_entries():
    assert per_call_value("eta", [0.3, 0.3]) == 0.3 and per_call_value("eta", 0.3) == 0.3
    with pytest.raises(ValueError, match="eta"):
        per_call_value("eta", [])


@pytest.mark.parametrize("name", ["face_clip_hidden_states", "faceid_embeds", "face_clip_image"])
def test_ipa_refuses_face_and_no_face_in_one_call(name):
    face = {"face_clip_hidden_states": torch.zeros(1, 257, 1280), "faceid_embeds": torch.zeros(512), "face_clip_image": torch.zeros(3, 32, 32)}[name]
    with pytest.raises(ValueError, match="with and without a face"):
        _pipe("ipa")(**_kw(**{name: [face, None, face]}))


@pytest.mark.parametrize("kind", KINDS)
def test_shard_over_ranks_with_several_requests_is_not_implemented(kind):
    with pytest.raises(NotImplementedError, match="shard_over_ranks"):
        _pipe(kind)(**_kw(shard_over_ranks=True))


def test_unipc_refuses_differing_guidance():
    with pytest.raises(ValueError, match="UniPC"):
        _pipe("base", unipc=True)(**_kw(guidance_scale=[5.0, 7.5, 9.0]))
    # uniform guidance is one scale per call: accepted by validation
    assert request_count(dict(prompt_embeds=torch.zeros(3, 77, 64), guidance_scale=[7.5, 7.5, 7.5]), scheduler=_sched(True)) == 3


def test_guidance_at_most_one_in_any_request_is_refused():
    with pytest.raises(NotImplementedError, match="guidance_scale <= 1"):
        _pipe("base")(**_kw(guidance_scale=[5.0, 1.0, 7.5]))


def test_request_count_inference():
    assert request_count(dict(prompt="a dress", prompt_embeds=None, ref_image_latents=torch.zeros(1, 4, 8, 8))) == 1
    assert request_count(dict(prompt=["a", "b"], ref_image_latents=torch.zeros(1, 4, 8, 8))) == 2          # one garment shared
    assert request_count(dict(prompt="a", ref_image_latents=torch.zeros(4, 4, 8, 8), negative_prompt=["x"] * 4)) == 4
    assert request_count(dict(ref_clip_hidden_states=torch.zeros(257, 1280))) == 1                          # unbatched tensor: one entry
    with pytest.raises(ValueError, match="negative_prompt"):
        request_count(dict(prompt=["a", "b", "c"], negative_prompt=["x", "y"]))
    assert per_request_floats("guidance_scale", 7.5, 3) == [7.5] * 3
    assert per_request_floats("guidance_scale", (5, 6, 7), 3) == [5.0, 6.0, 7.0]


def test_request_layout_maps_rows():
    lay = RequestLayout(3, 2)
    assert lay.rows == 6
    assert [lay.request_of_row(b) for b in range(12)] == [0, 0, 1, 1, 2, 2] * 2
    # text context [3 prompts; 3 negatives]: cond row b -> prompt b // n, uncond row 6 + j -> negative 3 + j // n
    assert [lay.ehs_row(b) for b in range(12)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    # ... which is what the processors' kv batch divisor computes (rows / context rows)
    pe, ne = torch.arange(3.0).view(3, 1, 1), 10 + torch.arange(3.0).view(3, 1, 1)
    ctx = lay.text_context(pe, ne)
    bdiv = 12 // ctx.shape[0]
    assert [int(ctx[b // bdiv]) for b in range(12)] == [0, 0, 1, 1, 2, 2, 10, 10, 11, 11, 12, 12]
    assert [lay.garment_of_row(b) for b in range(12)] == [0, 0, 1, 1, 2, 2] + [None] * 6
    assert lay.per_row([5.0, 7.5, 9.0]).tolist() == [5.0, 5.0, 7.5, 7.5, 9.0, 9.0]
    assert lay.expand(torch.arange(3.0).view(3, 1), "x").view(-1).tolist() == [0, 0, 1, 1, 2, 2]
    assert lay.expand(torch.ones(1, 2), "x").shape == (6, 2) and lay.expand(torch.ones(6, 2), "x").shape == (6, 2)
    with pytest.raises(ValueError, match="x has 4 rows"):
        lay.expand(torch.ones(4, 2), "x")
    # one request: today's [prompt, negative] context (first rows), kv divisor = images per request
    one = RequestLayout(1, 4)
    ctx1 = one.text_context(torch.zeros(2, 77, 8), torch.ones(2, 77, 8))
    assert ctx1.shape == (2, 77, 8) and ctx1[0].eq(0).all() and ctx1[1].eq(1).all()
    assert [one.ehs_row(b) for b in range(8)] == [0] * 4 + [1] * 4


def test_processor_maps_cond_rows_to_garments_in_every_block():
    """under sa_pair_layout the garment batch divisor is computed over the COND rows -- the same b // (B_cond / R) for the 2B-row blocks
    and for the first (pair-half) block, which sees the B cond rows only"""
    from imagdressing_amd.adapter.attention_processor import RefSAttnProcessor2_0
    proc = RefSAttnProcessor2_0("down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor", 80)
    ref = torch.zeros(3, 16, 80)
    B_cond = 6                         # R = 3 requests x n = 2 images
    assert proc._garment_bdiv(B_cond, ref) == 2
    with pytest.raises(ValueError, match="does not divide"):
        proc._garment_bdiv(4, ref)


# ---- the C entry point ----
def _declared():
    text = open(os.path.join(ROOT, "include", "imagdressing_hip.h")).read()
    return set(re.findall(r"\b(imd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


@pytest.fixture(scope="module")
def lib():
    from imagdressing_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_rows_step_declared_bound_exported(lib):
    from imagdressing_amd import _lib
    assert "imd_ddim_cfg_step_rows" in _declared()
    assert "imd_ddim_cfg_step_rows" in _lib.SYMBOLS
    assert hasattr(lib, "imd_ddim_cfg_step_rows")
    assert lib.imd_abi_version() == 9
    assert "imd_ddim_cfg_step_rows" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_rows_step_refuses_foreign_struct_size_without_gpu(lib):
    from imagdressing_amd import _lib
    p = _lib.DdimParams()
    assert p.struct_bytes == ctypes.sizeof(_lib.DdimParams)
    g = (ctypes.c_float * 4)()
    p.struct_bytes = ctypes.sizeof(_lib.DdimParams) - 8
    assert lib.imd_ddim_cfg_step_rows(ctypes.byref(p), ctypes.addressof(g), None) != 0
    assert b"ddim_cfg_step_rows" in lib.imd_last_error() and b"parameter block is" in lib.imd_last_error()
    p.struct_bytes = ctypes.sizeof(_lib.DdimParams)                      # right size, null pointers: refused before any launch
    assert lib.imd_ddim_cfg_step_rows(ctypes.byref(p), None, None) != 0
    assert b"null pointer" in lib.imd_last_error()
    assert lib.imd_ddim_cfg_step_rows(None, ctypes.addressof(g), None) != 0 and b"null params" in lib.imd_last_error()


def test_per_row_step_has_no_cpu_path():
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    with pytest.raises(ImdError):              # CPU tensors: refused, no fallback
        ops.ddim_cfg_step(torch.zeros(2, 4, 4), torch.zeros(4, 4, 4), None, guidance=torch.ones(2))
