"""Shared machinery of the four ``IMAGDressing_v1`` pipeline classes.

The reference pipelines subclass diffusers' ``StableDiffusionPipeline`` /
``StableDiffusionControlNetInpaintPipeline`` (un-vendored).  Here the pipeline is a plain class that
keeps the reference's constructor kwargs, ``__call__`` kwargs, ``set_scale`` / ``set_ipa_scale`` and
return type, and re-designs the loop (IMAGDressing_v1_pipeline.py:463-541) MI355X-first:

* the reference issues two batch-1 UNet calls per step (cond with garment tokens, uncond without);
  here ONE UNet call runs a [2B] batch -- rows [0, B) cond, rows [B, 2B) uncond -- with the garment
  branch switched per row (``sa_batch_mask``), for B images that share the garment;
* garment features are harvested once per garment from the garment UNet run at batch 1 (the
  reference runs it at batch 2 and discards half, quirk 8 of SURVEY.md), and their K/V projections
  are cached inside the processors for the whole loop;
* CFG + DDIM step + (inpaint blend) + the next step's UNet input are one elementwise kernel over
  an fp32 latent state;
* under ``torch.distributed`` the B images are sharded over ranks and the garment features are
  broadcast from rank 0 (one collective per garment, none in the loop).

Encoders outside the hot path (CLIP text / vision, VAE -- SURVEY.md 8f "next") are duck-typed torch
modules supplied by the caller, or bypassed with pre-computed tensors (``prompt_embeds``,
``negative_prompt_embeds``, ``ref_clip_hidden_states``, ``ref_image_latents``, ``latents``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence, Union

import torch

from ... import ops
from ...adapter.attention_processor import (IPAttnProcessor2_0, LoRAIPAttnProcessor2_0, LoraRefSAttnProcessor2_0,
                                            RefSAttnProcessor2_0)
from ...scheduler import unipc_fused
from ...unet import DeepCache, nchw_to_nhwc8

bf16 = torch.bfloat16


@dataclass
class StableDiffusionPipelineOutput:
    images: Any
    nsfw_content_detected: Optional[List[bool]] = None


def randn_tensor(shape, generator=None, device=None, dtype=torch.float32):
    """diffusers ``randn_tensor``: CPU generators sample on the CPU (cross-vendor reproducible)."""
    device = torch.device(device or "cpu")
    if isinstance(generator, (list, tuple)):
        return torch.cat([randn_tensor((1,) + tuple(shape[1:]), g, device, dtype) for g in generator], 0)
    gdev = generator.device if generator is not None else device
    if gdev.type != device.type:
        return torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


def deepcache_plan(n_calls: int, cache_interval: int) -> List[bool]:
    """Which UNet calls of a pipeline call are full (True) and which shallow (``enable_deepcache``): call c, counted from the first
    EXECUTED call (``strength`` < 1 skips the head of the schedule; PNDM's extra call is just another index), is full iff
    c % cache_interval == 0.  Call 0 is always full: it fills the feature cache and the processors' step-invariant K / V caches."""
    cache_interval = int(cache_interval)
    if cache_interval < 1:
        raise ValueError(f"cache_interval must be >= 1, got {cache_interval}")
    return [c % cache_interval == 0 for c in range(int(n_calls))]


class PipelineBase:
    vae_scale_factor = 8

    def _init_common(self, *, vae, reference_unet, unet, tokenizer, text_encoder, image_encoder, ImgProj, scheduler,
                     safety_checker=None, feature_extractor=None, controlnet=None):
        from ...hub import PendingModel

        def ready(m):          # a ``from_pretrained`` handle that never met ``.to(device=...)``: build it now (default device)
            return m._build() if isinstance(m, PendingModel) else m
        if isinstance(controlnet, (list, tuple)):          # controlnet=[a, b]: wrapped like diffusers does
            from ...unet import MultiControlNetModel
            controlnet = MultiControlNetModel([ready(n) for n in controlnet])
        vae, reference_unet, unet, controlnet = ready(vae), ready(reference_unet), ready(unet), ready(controlnet)
        text_encoder, image_encoder = ready(text_encoder), ready(image_encoder)
        for role, m in (("unet", unet), ("reference_unet", reference_unet), ("controlnet", controlnet)):
            if isinstance(m, torch.nn.Module) and not hasattr(m, "forward_nhwc"):        # e.g. a stock diffusers UNet2DConditionModel
                raise TypeError(
                    f"IMAGDressing_v1({role}=...): got a {type(m).__module__}.{type(m).__name__}.  These pipelines drive the MI355X engine "
                    "UNet (imagdressing_amd.unet.UNet2DConditionModel / ControlNetModel; NHWC, fused CFG batch) -- build it from the same "
                    "checkpoint with `UNet2DConditionModel.from_pretrained(dir, subfolder='unet').to(dtype=torch.float16, device='cuda')` "
                    "imported from imagdressing_amd.unet, or put <repo>/compat on sys.path so that `from diffusers import "
                    "UNet2DConditionModel` resolves to it (INTEGRATION.md section 1).  The attention PROCESSORS alone also work on a "
                    "stock diffusers UNet (unet.set_attn_processor), but then the stock diffusers pipeline has to drive it.")
        self.vae, self.reference_unet, self.unet = vae, reference_unet, unet
        self.tokenizer, self.text_encoder, self.image_encoder = tokenizer, text_encoder, image_encoder
        self.ImgProj, self.scheduler, self.controlnet = ImgProj, scheduler, controlnet
        # the reference scripts pass the *classes* here (inference_IMAGdressing.py:133-134): tolerated, unused
        self.safety_checker, self.feature_extractor = safety_checker, feature_extractor
        self._cross_attention_kwargs = None
        self._garment_cache = None
        if vae is not None and hasattr(vae, "config") and hasattr(vae.config, "block_out_channels"):
            self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1)

    # ---- one ControlNet or several (unet.MultiControlNetModel) ----
    def _control_nets(self) -> list:
        """the ControlNets of this pipeline, in order: none, the one given, or the nets of a ``MultiControlNetModel``"""
        cn = getattr(self, "controlnet", None)
        if cn is None:
            return []
        return list(cn.nets) if hasattr(cn, "nets") else [cn]

    def _single_controlnet(self):
        """what the one-net routes drive: the net itself, also where it came wrapped (``MultiControlNetModel([a])`` is ``a``)"""
        nets = self._control_nets()
        return nets[0] if len(nets) == 1 else getattr(self, "controlnet", None)

    def _refuse_multi(self, what: str):
        K = len(self._control_nets())
        if K >= 2:
            raise NotImplementedError(f"{what} on a pipeline with {K} ControlNets: the mix of several nets' residuals "
                                      "(imd_residual_mix_rows) is built for whole calls on one rank; use one ControlNet here")

    # ---- reference surface ----
    @property
    def cross_attention_kwargs(self):
        return self._cross_attention_kwargs

    @property
    def device(self):
        return self.unet.device

    _execution_device = device

    def set_tuning(self, attn_variant: Optional[int] = None, attn_xcd: Optional[bool] = None, gemm_flags: Optional[int] = None):
        """Kernel tuning of THIS pipeline's launches (head-dim-40 attention variant, XCD-aware attention work order, GEMM tuning bits 0..4),
        carried per call in the params blocks (``ops.tuning_scope``, ``IMD_TUNING_PER_CALL``): two pipelines of one process may differ and
        the library's process-wide knobs (``imd_set_tuning``) are not touched.  All None (the default) = the process-wide settings."""
        self._tuning = dict(attn_variant=attn_variant, attn_xcd=attn_xcd, gemm_flags=gemm_flags)
        self.release_step_graph()            # a captured step graph bakes its kernels in
        return self

    def enable_step_graph(self, flag: bool = True):
        """Opt in to HIP-graph replay of the denoising step (see ``denoise``) -- DDIM and the deterministic samplers of the fused
        sampler step (DPM-Solver++, Euler, PNDM): same kernels, same arithmetic, one graph launch per step instead of ~500 kernel
        launches.  Worth it where the loop is host-bound (small batches); ignored for UniPC (unless ``scheduler.enable_fused_step()``:
        its one-launch step replays like the others), Euler-ancestral (unless ``enable_device_noise()``: its noise launch is then part
        of the captured step), step callbacks, traces,
        per-step ControlNet gating and while ``enable_deepcache`` is on."""
        self._step_graph = bool(flag)
        if not flag:
            self.release_step_graph()
        return self

    def release_step_graph(self):
        """Drop the captured step graph, the side stream it was recorded on and every scratch buffer keyed by that stream
        (``ops.clear_workspaces(stream=...)``): the graph pins a private memory pool, and the per-stream workspaces (attention operand
        buffers, GroupNorm partials, a >= 16 MB split-K slab) would otherwise live as long as the process."""
        side = self.__dict__.pop("_graph_stream", None)
        self.__dict__.pop("_last_step_graph", None)
        if side is not None:
            side.synchronize()
            ops.clear_workspaces(stream=side.cuda_stream)

    def __del__(self):
        try:
            self.release_step_graph()
        except Exception:        # noqa: BLE001  (interpreter shutdown)
            pass

    def enable_deepcache(self, cache_interval: int = 3, depth: int = 1):
        """Opt in to step-to-step feature caching (DeepCache, Ma et al., CVPR 2024; ``unet.DeepCache``): UNet call c of a pipeline call
        is a full forward iff c % ``cache_interval`` == 0 (``deepcache_plan``); every other call recomputes only conv_in, the first
        ``depth`` - 1 layers of the first down block and the last ``depth`` layers of the last up block around the deep feature the last
        full call stored, and the ControlNet computes only the residuals those layers read.  The result CHANGES (that is the point);
        what it does to image quality with real checkpoints is unmeasured, hence off by default.  ``cache_interval`` = 1 computes what
        the switch-off loop computes.  While the switch is on, ``enable_step_graph`` is ignored (the call runs eagerly).  The cache
        lives for one denoising call."""
        if int(cache_interval) < 1:
            raise ValueError(f"cache_interval must be >= 1, got {cache_interval}")
        layers = getattr(getattr(self.unet, "config", None), "layers_per_block", 2)
        if not 1 <= int(depth) <= layers + 1:
            raise ValueError(f"depth must be in 1 .. {layers + 1} (layers_per_block + 1), got {depth}")
        self._deepcache = (int(cache_interval), int(depth))
        return self

    def disable_deepcache(self):
        self._deepcache = None
        return self

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """Opt in to FreeU (Si et al., CVPR 2024; diffusers' ``pipe.enable_freeu(s1, s2, b1, b2)``) on the denoising UNet
        (``UNet2DConditionModel.enable_freeu``): the backbone's lower channel half is scaled by ``b1`` / ``b2`` and the skips are
        low-pass re-weighted by ``s1`` / ``s2`` at the first two up blocks, inside the launch that concatenates them.  No extra steps,
        no weights; the garment UNet and the ControlNet are untouched.  The result CHANGES (that is the point); what it does to image
        quality with real checkpoints is unmeasured, hence off by default.  All four values must be finite and > 0.  Composes with
        ``enable_step_graph`` (every call captures its own step), DeepCache, sessions and request batches."""
        if self.unet is None:
            raise ValueError("enable_freeu: this pipeline has no unet")
        self.unet.enable_freeu(s1, s2, b1, b2)
        return self

    def disable_freeu(self):
        if self.unet is None:
            raise ValueError("disable_freeu: this pipeline has no unet")
        self.unet.disable_freeu()
        return self

    def enable_device_image_io(self, flag: bool = True):
        """Opt in to image input and output on the GPU (``imagdressing_amd.image.DeviceImageProcessor``): PIL / uint8 pose, control,
        inpainting and mask images are resized (Pillow's Lanczos filter, bit for bit), scaled and laid out by ``imd_image_resample``
        instead of on one host thread, and ``output_type="pil" | "np"`` packs the decoder's NHWC output to uint8 on the device and copies
        one byte per channel value back instead of four.  No pixel changes; float tensor inputs and ``"pt"`` / ``"latent"`` outputs keep
        the host route.  Off by default."""
        self._device_image_io = bool(flag)
        return self

    def disable_device_image_io(self):
        return self.enable_device_image_io(False)

    def enable_request_adapter_scales(self, flag: bool = True):
        """Opt in to ``ipa_scale``, ``s_lora_scale`` and ``c_lora_scale`` PER REQUEST in a request-batched call of the IP-Adapter +
        ControlNet pipeline: each takes one value or one per request.  Each argument on its own: equal values (or a scalar) keep the
        folded route -- ``set_scale`` / ``set_ipa_scale``, LoRA folded into the weights, every launch and every bit as with the switch
        off; differing values ride in rows (``s_lora_rows`` / ``c_lora_rows`` / ``ip_scale_rows`` of the cross-attention kwargs) and the
        LoRA of those layers runs unfolded, y = [x | s_row (x D^T)] [W | U]^T: one ``imd_lora_expand_rows`` launch in front of each
        projection, whose K grows by the rank.  That route costs time (see README); grouping requests by equal scales avoids it.
        A request with all three at 0 gets the scale settings of the reference's no-face branch, which is how a call mixes requests
        with and without a face (face arguments themselves stay all-or-none).  Off by default: differing sequences then raise, as
        ever.  A no-op on the pipelines without LoRA / IP-Adapter processors (base, ControlNet, inpainting): they have none of the
        three arguments."""
        self._request_adapter_scales = bool(flag)
        return self

    def disable_request_adapter_scales(self):
        return self.enable_request_adapter_scales(False)

    def enable_request_control_scales(self, flag: bool = True):
        """Opt in to ``controlnet_conditioning_scale``, ``control_guidance_start`` and ``control_guidance_end`` PER REQUEST in a
        request-batched call of the ControlNet, IP-Adapter + ControlNet and inpainting pipelines (and in their sessions,
        ``open_session(control_rows=...)``): each takes one value or one per request.  The route is chosen once per call.  Requests
        whose (scale, start, end) triples all agree keep the folded route -- the scale is ``out_scale`` of the 13 zero-conv launches,
        every launch and every bit as with the switch off.  Otherwise the whole call takes the rows route: the zero convs run with
        ``out_scale`` = 1 and ONE ``imd_residual_scale_rows`` launch per step gives every batch row ``scale_r * keep_r[step]``; a
        row at 1.0 is not touched.  A residual is then 16-bit(s 16-bit(W x + b)) instead of 16-bit(s (W x + b)): at most one unit in the
        last place apart, equal where s is 1 (bf16: a power of two).  On the rows route ``enable_step_graph`` replays calls whose gate
        changes over the steps (the scale array is refreshed next to the coefficients).  Off by default: a differing list then raises
        and the window arguments read their first entry, as ever.  A no-op on the base pipeline, which has no ControlNet."""
        self._request_control_scales = bool(flag)
        return self

    def disable_request_control_scales(self):
        return self.enable_request_control_scales(False)

    def _multi_control(self, name: str, images, shard_over_ranks: bool):
        """K of a call that drives several ControlNets (0: it does not -- one net, none, or no control image), after the refusals"""
        K = len(self._control_nets())
        if K < 2 or images is None:
            return 0
        if shard_over_ranks:
            self._refuse_multi("shard_over_ranks=True")
        return K

    def _multi_control_plan(self, scale, start, end, K: int, R: int, steps: int):
        """``multi_rows`` of a call's ``control`` dict on K >= 2 nets: ``multi_control_plan`` under this pipeline's switch"""
        return multi_control_plan(scale, start, end, K, R, steps, per_request=getattr(self, "_request_control_scales", False))

    def _control_plan(self, scale, start, end, R: int, steps: int):
        """-> (scale, keep, rows) of a call's ``control`` dict: ``control_plan`` under this pipeline's switch"""
        return control_plan(scale, start, end, R, steps, per_request=getattr(self, "_request_control_scales", False))

    def enable_device_noise(self, flag: bool = True):
        """Opt in to noise that belongs to a REQUEST and is made on the device (``imd_noise_rows``, imagdressing_amd/noise.py): the
        initial latents (unless ``latents=`` is given), the per-step noise of Euler-ancestral and of ``eta`` > 0 (unless
        ``variance_noise=`` is given) and the inpainting blend noise become a pure function of (seed, image, draw, pixel) -- Philox4x32-10
        and Box-Muller, one launch for all rows.  The seed of request r: the keyword ``seed`` (an int in [0, 2^64), or a list with one
        per request), else ``generator[r].initial_seed()``, else 8 bytes of ``os.urandom``; the seeds used are left in
        ``pipe.last_seeds``.  A request then gets the same noise alone, in a request batch, under ``enable_step_graph`` (which now
        replays Euler-ancestral too) and in any slot of a session (``open_session``, which then admits Euler-ancestral and DDIM with
        ``eta`` > 0).  The result CHANGES: this is not torch's random stream, the noise is fp32 and not rounded to the UNet's element
        type, and its tails are cut at 5.77 sigma (a mass of about 1e-8); what that does to image quality with real checkpoints is
        unmeasured.  The VAE's posterior sample stays on torch.  Off by default: every launch, bit and refusal is then today's."""
        self._device_noise = bool(flag)
        return self

    def disable_device_noise(self):
        return self.enable_device_noise(False)

    def _request_noise(self, kwargs: Dict[str, Any], generator, R: int, images_per_request: int):
        """the :class:`imagdressing_amd.noise.RequestNoise` of this call (``enable_device_noise``), else None; ``seed=`` is read from
        the call's ``**kwargs`` like ``variance_noise``"""
        seed = kwargs.get("seed")
        if not getattr(self, "_device_noise", False):
            if seed is not None:
                raise ValueError("seed= is the request seed of the device noise source: call pipe.enable_device_noise() first "
                                 "(without it the noise comes from generator=, as ever)")
            return None
        from ...noise import RequestNoise, resolve_seeds
        self.last_seeds = resolve_seeds(seed, generator, R)
        return RequestNoise(self.last_seeds, images_per_request, self.device)

    def _shard_noise(self, plan, shard: bool):
        """the rows of ``plan`` that :meth:`_shard` leaves this rank"""
        if plan is None or not shard:
            return plan
        from ... import dist as imd_dist
        return plan.shard(imd_dist.shard_bounds(plan.rows))

    @staticmethod
    def _adapter_scales(name, value, R, neutral):
        """-> (the value the processors get through set_scale / set_ipa_scale, per-request values for the loop or None), like
        :meth:`_image_scales`: equal values (and a scalar) keep the folded route; differing ones ride in rows, the processors' own
        attribute at ``neutral`` (the rows are read instead of it)."""
        vals = per_request_floats(name, value, R)
        return (vals[0], None) if len(set(vals)) == 1 else (neutral, vals)

    def _image_processor(self):
        from ...image import DeviceImageProcessor
        proc = self.__dict__.get("_image_proc")
        if proc is None or proc.device != self.device or proc.dtype != self.unet.dtype:
            proc = self._image_proc = DeviceImageProcessor(self.device, self.unet.dtype)
        return proc

    def _image_tensor(self, image, device, normalize: bool, size=None, multiple: int = 8, layout: str = "nchw", binarize: bool = False):
        """-> (tensor, (height, width)).  ``to_image_tensor`` (fp32 NCHW) -- or, with device image I/O enabled and PIL / uint8 images
        that need no nearest-neighbour resize, the same values from the GPU: ``layout="nchw"`` fp32 [B, 3 | 1, H, W]; ``"nhwc8"``: the
        engines' [B, H, W, 8] (what ``nchw_to_nhwc8`` makes of it).  The size is returned beside the tensor because the two layouts
        keep it in different places.  ``binarize`` (masks) thresholds at 0.5 on the device; the host route leaves that to the caller."""
        if getattr(self, "_device_image_io", False) and torch.device(device).type == "cuda":
            ims = list(image) if isinstance(image, (list, tuple)) else [image]
            hw = None if size is None else (int(size[0]) // multiple * multiple, int(size[1]) // multiple * multiple)

            def on_device(im):
                if hasattr(im, "convert") and hasattr(im, "resize"):
                    return True                # PIL: Lanczos to ``hw``, as the host route
                # uint8 [H, W, 3] arrays: the host route resizes those with F.interpolate (nearest) -- only unresized ones come here
                return (not isinstance(im, torch.Tensor) and getattr(im, "dtype", None) == "uint8" and getattr(im, "ndim", 0) == 3
                        and im.shape[-1] == 3 and (hw is None or tuple(im.shape[:2]) == hw))
            if ims and all(on_device(im) for im in ims):
                gray = binarize and all(getattr(im, "mode", None) in ("1", "L") for im in ims)     # (their RGB conversion repeats the one channel)
                t = self._image_processor().preprocess(ims, size=size, resample="lanczos", out=layout, normalize=normalize,
                                                       binarize=binarize, multiple=multiple, mode="L" if gray else "RGB")
                return t, (tuple(t.shape[1:3]) if layout == "nhwc8" else tuple(t.shape[-2:]))
        t = to_image_tensor(image, device, normalize, size=size, multiple=multiple)
        return t, tuple(t.shape[-2:])

    def enable_vae_slicing(self):
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    def progress_bar(self, iterable=None, total=None):
        try:
            from tqdm.auto import tqdm
            return tqdm(iterable, total=total, disable=getattr(self, "_progress_disabled", True))
        except Exception:   # pragma: no cover
            class _N:
                def __enter__(s): return s
                def __exit__(s, *a): return False
                def update(s, *a): pass
            return _N()

    def set_progress_bar_config(self, disable=False, **kw):
        self._progress_disabled = disable

    # ---- encoders outside the hot path (duck-typed torch modules) ----
    def encode_prompt(self, prompt, device, num_images_per_prompt=1, do_classifier_free_guidance=True,
                      negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None, clip_skip=None):
        def enc(text):
            if self.tokenizer is None or self.text_encoder is None:
                raise ValueError("no tokenizer/text_encoder: pass prompt_embeds / negative_prompt_embeds")
            ids = self.tokenizer(text, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                                 return_tensors="pt").input_ids
            return self.text_encoder(ids.to(device))[0]
        if prompt_embeds is None:
            prompt_embeds = enc(prompt)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt_embeds = enc(negative_prompt if negative_prompt is not None else "")
        return prompt_embeds, negative_prompt_embeds

    def _clip_hidden(self, clip_image, device):
        dt = next(self.image_encoder.parameters()).dtype
        return self.image_encoder(clip_image.to(device, dtype=dt), output_hidden_states=True).hidden_states[-2]

    def prepare_latents(self, batch_size, num_channels_latents, width, height, dtype, device, generator, latents=None, noise_plan=None):
        # NB the reference passes (width, height) in this order to a (height, width) signature, and so keeps
        # shape [B, 4, width//8, height//8] semantics consistent with its own call (:440-448); we take them named.
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None and noise_plan is not None:          # enable_device_noise: draw 0 of every request, one launch
            if noise_plan.rows != batch_size or num_channels_latents != 4:
                raise ValueError(f"device noise: {noise_plan.rows} keyed rows for latents {shape}")
            latents = noise_plan.initial(shape[2], shape[3])
        if latents is None:
            latents = randn_tensor(shape, generator=generator, device=device, dtype=torch.float32)
        return latents.to(device=device, dtype=torch.float32) * self.scheduler.init_noise_sigma

    # ---- garment features (A2 of SURVEY 8a) ----
    @torch.no_grad()
    def garment_features(self, ref_image_latents: torch.Tensor, cloth_proj_embed: torch.Tensor, garments: int = 1) -> Dict[str, torch.Tensor]:
        """Garment UNet once at t = 0 with the 16 resampler tokens as context; returns the (post-LayerNorm)
        input of every attention layer, [1, M, C] each (IMAGDressing_v1_pipeline.py:465-480) -- or [G, M, C] for ``garments`` = G
        distinct garments of a request-batched call (one garment-UNet forward at batch G)."""
        with ops.tuning_scope(**(getattr(self, "_tuning", None) or {})):
            return self._garment_features(ref_image_latents, cloth_proj_embed, garments)

    def _garment_features(self, ref_image_latents, cloth_proj_embed, garments: int = 1):
        """``garments`` = G > 1 (a request-batched call): ``ref_image_latents`` / ``cloth_proj_embed`` hold one row per garment and the
        garment UNet runs ONE forward at batch G -> [G, M, C] per layer (row g = garment g)."""
        dt = self.reference_unet.dtype
        if garments > 1:
            if ref_image_latents.shape[0] != garments or cloth_proj_embed.shape[0] != garments:
                raise ValueError(f"{garments} garments: ref_image_latents has {ref_image_latents.shape[0]} rows and the garment tokens "
                                 f"{cloth_proj_embed.shape[0]}")
            x = nchw_to_nhwc8(ref_image_latents.to(self.device), dt)
            ehs = cloth_proj_embed.to(device=self.device, dtype=dt).contiguous()
        else:
            x = nchw_to_nhwc8(ref_image_latents[:1].to(self.device), dt)
            ehs = cloth_proj_embed[-1:].to(device=self.device, dtype=dt).contiguous()     # the cond half ([1] of the CFG pair)
        self.reference_unet.forward_nhwc(x, 0, ehs)
        out = {}
        for name, proc in self.reference_unet.attn_processors.items():
            out[name] = proc.cache["hidden_states"]
        return out

    # ---- the loop ----
    @torch.no_grad()
    def denoise(self, **kw) -> torch.Tensor:
        """:meth:`_denoise` inside this pipeline's tuning scope (:meth:`set_tuning`)."""
        with ops.tuning_scope(**(getattr(self, "_tuning", None) or {})):
            return self._denoise(**kw)

    def _denoise(self, *, latents: torch.Tensor, prompt_embeds: torch.Tensor, negative_prompt_embeds: torch.Tensor,
                sa_hidden_states: Dict[str, torch.Tensor], num_inference_steps: int, guidance_scale: Union[float, Sequence[float]],
                control: Optional[dict] = None, inpaint: Optional[dict] = None,
                callback: Optional[Callable] = None, callback_steps: int = 1, trace: Optional[list] = None,
                eta: float = 0.0, generator=None, variance_noise: Optional[List[torch.Tensor]] = None, t_start: int = 0,
                requests: int = 1, image_scale: Optional[Sequence[float]] = None,
                adapter_rows: Optional[Dict[str, Optional[Sequence[float]]]] = None,
                guidance_rescale: Union[float, Sequence[float]] = 0.0, noise_plan=None) -> torch.Tensor:
        """latents [B, 4, h, w] fp32 -> final latents [B, 4, h, w] fp32.

        ``requests`` = R > 1: a request-batched call (:class:`RequestLayout`) -- latent rows [r n, (r+1) n) belong to request r
        (n = B / R); ``prompt_embeds`` / ``negative_prompt_embeds`` (and the ControlNet's) hold R rows (or 1, shared); garment
        tensors in ``sa_hidden_states`` hold R rows (or 1, shared); ``guidance_scale`` may be a sequence of R values (the per-row
        fused step, ``imd_ddim_cfg_step_rows``, when they differ) and ``image_scale`` a sequence of R garment-branch weights
        (carried in the ``sa_batch_mask`` rows; the processors' own ``scale`` is then expected to be 1).  ``control["image"]`` and
        the ``inpaint`` tensors hold 1, R or B rows.  ``adapter_rows`` (``enable_request_adapter_scales``): for each of ``s_lora_rows``,
        ``c_lora_rows``, ``ip_scale_rows`` None or R values -- they become fp32 [2B] device tensors in the cross-attention kwargs, a
        request's value on all its rows, cond and uncond alike (the reference's processors do not look at the CFG half).

        The scheduler decides the step: DDIM (``imd_ddim_cfg_step``), a scheduler with a ``plan`` method -- DPM-Solver++, Euler,
        Euler-ancestral, PNDM (scheduler.py) -- one ``imd_sampler_step`` per step with the same guidance / blend / graph-replay
        features (Euler-ancestral draws its per-step noise like ``eta`` > 0 below and runs eagerly), or UniPC: ``step_guided`` (three
        ``imd_lincomb`` launches, one guidance scale, no blend, no replay) unless ``scheduler.enable_fused_step()``, which gives it
        one ``imd_unipc_step`` per step and every feature of the ``plan`` samplers.
        ``eta`` > 0 (DDIM only; other schedulers ignore it, like ``prepare_extra_step_kwargs``, IMAGDressing_v1_pipeline.py:102-119):
        the stochastic step, noise per step = ``variance_noise[i]`` [B, 4, h, w] or a draw of that shape in the UNet's element type
        from ``generator`` (what ``DDIMScheduler.step`` does with the reference's ``noise_pred``).
        ``t_start``: skip the first t_start timesteps of the schedule (inpainting ``strength`` < 1,
        ..._controlnet_inpainting.py:316-319 -> diffusers ``get_timesteps``); ``latents`` is then the noised image latent.

        ``guidance_rescale``: the CFG rescale of Lin et al. 2023, section 3.4 (diffusers' ``rescale_noise_cfg``), one value in [0, 1] per
        call or per request.  All 0: nothing new happens.  Otherwise ONE ``imd_guidance_rescale`` launch between the UNet and the step
        writes the rescaled guided prediction into both CFG halves of eps, so every fused step recovers it unchanged -- eager or captured;
        a host-stepped UniPC (``step_guided``) refuses it.

        ``noise_plan`` (``enable_device_noise``; a ``noise.RequestNoise`` of B rows): the per-step noise of a stochastic step, unless
        ``variance_noise`` is given, is draw 1 + t_start + i of each row's request, written in fp32 by ONE ``imd_noise_rows`` launch in
        front of the step into a buffer at a fixed address; the key rows of the whole call are uploaded once.  Euler-ancestral then
        replays under ``enable_step_graph`` (the launch is part of the captured step; the host refreshes 32 bytes of key per row next
        to the coefficients).  DDIM with ``eta`` > 0 stays eager: its step refuses ``var_noise`` with device coefficients.

        ``control`` = dict(image=[1|B, 3, H, W] in [0,1] or NHWC8 bf16, prompt_embeds=[1,77,768],
        negative_prompt_embeds=[1,77,768], scale=float, keep=[float]*steps)
        ``inpaint`` = dict(mask=[B|1,1,h,w], image_latents=[B|1,4,h,w], noise=[B,4,h,w]) and, for ``soft_mask``, optionally
        ``release`` = integer [1|R|B, h, w] (``image.mask_release_reference``: the step from which a pixel is free) with ``soft_rows`` =
        R bools (None: every request): ONE ``imd_soft_mask_rows`` launch in front of every step writes the 0 / 1 mask ``k >= release``
        into the soft requests' rows of the mask buffer, k from a [calls][B] table uploaded once (:func:`soft_step_table`); a captured
        step reads k from a fixed buffer refreshed next to the coefficients.  The hard requests' rows keep ``mask``.
        """
        dev = self.device
        B, Cl, h, w = latents.shape
        HW = h * w
        lay = RequestLayout(int(requests), B // max(int(requests), 1))
        if lay.requests < 1 or lay.rows != B:
            raise ValueError(f"{B} latent rows cannot be split into {requests} requests")
        gs = per_request_floats("guidance_scale", guidance_scale, lay.requests)
        unipc = unipc_fused(self.scheduler)                       # UniPC with enable_fused_step(): one imd_unipc_step per step
        multistep = hasattr(self.scheduler, "step_guided") and not unipc      # UniPC: latent updates are host-computed linear combinations
        fused = (not multistep and hasattr(self.scheduler, "plan")) or unipc  # DPM-Solver++ / Euler / Euler-ancestral / PNDM: one imd_sampler_step per step
        if len(set(gs)) > 1 and multistep:
            raise ValueError("guidance_scale differs between the requests: the per-request guidance step is the fused DDIM step; "
                             "UniPC takes one guidance scale per call")
        # uniform guidance: the scalar step (a single-request call is unchanged); otherwise one fp32 value per latent row, alive for the
        # whole call (a captured step graph reads it at every replay)
        g_arg = gs[0] if len(set(gs)) == 1 else lay.per_row(gs).to(dev)
        # guidance_rescale: None (every value 0: no tensor, no launch), the scalar, or one fp32 value per latent row alive like g_arg
        phis = guidance_rescale_values(guidance_rescale, lay.requests)
        phi_arg = None if not any(phis) else (phis[0] if len(set(phis)) == 1 else lay.per_row(phis).to(dev))
        if phi_arg is not None and multistep:
            raise NotImplementedError("guidance_rescale with the host-stepped UniPC (step_guided): the rescale runs in front of a fused "
                                      "step; call scheduler.enable_fused_step() first")
        sch = self.scheduler
        sch.set_timesteps(num_inference_steps, device=dev)
        if fused:          # fractional timesteps (Euler, "linspace" spacing or Karras sigmas) reach the time embedding unrounded
            timesteps = [t.item() for t in sch.timesteps][int(t_start):]
        else:
            timesteps = [int(t) for t in sch.timesteps][int(t_start) * getattr(sch, "order", 1):]
        if not timesteps:
            raise ValueError(f"no denoising steps left (num_inference_steps={num_inference_steps}, t_start={t_start})")
        z = latents.to(device=dev, dtype=torch.float32).permute(0, 2, 3, 1).reshape(B, HW, Cl).contiguous()
        dt = self.unet.dtype
        x_in = torch.zeros(2 * B, h, w, 8, dtype=dt, device=dev)
        x_in[..., :Cl] = torch.cat([z, z]).view(2 * B, h, w, Cl)
        if fused and sch.input_scale(int(t_start)) != 1.0:          # scale_model_input of the first step; later inputs come scaled out of the step
            x_in[..., :Cl] = (torch.cat([z, z]) * sch.input_scale(int(t_start))).view(2 * B, h, w, Cl)
        # rows [0,B): prompt (+garment), rows [B,2B): negative prompt, no garment -> ehs rows shared per half (R > 1: [R prompts; R negatives],
        # the processors' kv bdiv = n then maps cond row b to prompt b // n and uncond row B + j to negative j // n -- RequestLayout.ehs_row)
        ehs = lay.text_context(prompt_embeds, negative_prompt_embeds).to(device=dev, dtype=dt).contiguous()
        cond_w = torch.ones(B) if image_scale is None else lay.per_row(per_request_floats("image_scale", image_scale, lay.requests))
        mask_rows = torch.cat([cond_w, torch.zeros(B)]).to(device=dev, dtype=torch.float32)
        # sa_pair_layout: the mask above IS "garment on for rows [0, B), off for rows [B, 2B)" -- together with cfg_pair (identical latents in
        # the two halves) it lets the engine run the first hybrid block's self-attention phase once per image (unet.call_pair_half)
        cak = {"sa_hidden_states": sa_hidden_states, "sa_batch_mask": mask_rows, "sa_pair_layout": True}
        for key, vals in (adapter_rows or {}).items():          # alive for the whole call (a captured step graph reads them at every replay)
            if vals is not None:
                cak[key] = lay.per_row(per_request_floats(key, vals, lay.requests)).repeat(2).to(device=dev, dtype=torch.float32).contiguous()
        ctrl_img = ctrl_ehs = None
        # control["multi_rows"]: a call on K >= 2 ControlNets -- control["image"] is then a list of K images, one per net
        multi = control is not None and control.get("multi_rows") is not None
        if control is not None:
            def control_image(img):
                if lay.requests > 1 and img.shape[0] > 1:          # one control image per request (or per image): the ControlNet batch is 2B rows
                    img = lay.expand(img, "control image").repeat(2, *([1] * (img.dim() - 1)))
                return img if (img.dim() == 4 and img.shape[-1] == 8 and img.dtype == dt) else nchw_to_nhwc8(img.to(dev), dt)
            ctrl_img = [control_image(img) for img in control["image"]] if multi else control_image(control["image"])
            ctrl_ehs = lay.text_context(control["prompt_embeds"], control["negative_prompt_embeds"]).to(device=dev, dtype=dt).contiguous()
        inp = None
        if inpaint is not None:
            def nhwc(t, c):
                t = t.to(device=dev, dtype=torch.float32)
                if t.shape[0] != B:
                    t = t.expand(B, -1, -1, -1) if t.shape[0] == 1 else lay.expand(t, "inpaint input")
                return t.permute(0, 2, 3, 1).reshape(B, HW, c).contiguous()
            inp = dict(mask=nhwc(inpaint["mask"], 1).view(B, HW).contiguous(), z_img=nhwc(inpaint["image_latents"], Cl),
                       noise=nhwc(inpaint["noise"], Cl))
        if multistep and inp is not None:
            raise NotImplementedError("the inpainting blend is defined on the DDIM step (…inpainting.py:487-500)")       # (and on imd_sampler_step)
        # soft_mask: the rows of the soft requests get their 0 / 1 mask from the release steps in front of every step; the mask buffer
        # stays at its one address, the hard rows keep what was filled in above.  The step of every call is known before the first
        # launch: one [calls][B] table for the whole call, -1 for a hard row.  No soft row: nothing is allocated, uploaded or launched.
        soft = None
        if inp is not None and inpaint.get("release") is not None:
            flags = inpaint.get("soft_rows")
            flags = [True] * lay.requests if flags is None else [bool(f) for f in flags]
            if len(flags) != lay.requests:
                raise ValueError(f"inpaint soft_rows has {len(flags)} entries for {lay.requests} requests")
            if any(flags):
                rel = torch.as_tensor(inpaint["release"])
                if rel.is_floating_point() or rel.dtype == torch.bool or rel.dim() != 3 or tuple(rel.shape[1:]) != (h, w):
                    raise ValueError(f"inpaint release: expected an integer [1 | R | B, {h}, {w}] tensor, got {rel.dtype} {tuple(rel.shape)}")
                rel = rel.to(dev)
                if rel.dtype == torch.uint16:          # (the bits, as int16: the type torch expands and repeats on every device)
                    rel = rel.view(torch.int16)
                else:
                    rel = rel.to(torch.int64)
                    lo, hi = int(rel.min()), int(rel.max())
                    if lo < 0 or hi > ops.RELEASE_MAX_STEPS:
                        raise ValueError(f"inpaint release: a release step is in [0, {ops.RELEASE_MAX_STEPS}], got values from {lo} to {hi}")
                    rel = torch.where(rel >= 32768, rel - 65536, rel).to(torch.int16)
                rel = lay.expand(rel, "inpaint release").reshape(B, HW).contiguous().view(torch.uint16)
                # the launches write the mask at every step: the loop's buffer must not be the caller's tensor (an fp32 mask of B rows
                # on the device passes through nhwc() without a copy)
                inp["mask"] = inp["mask"].clone()
                # executed schedule positions: PNDM's run makes one UNet call more than it has positions
                positions = len(timesteps) - ((len(sch.timesteps) - int(num_inference_steps)) if fused else 0)
                table = soft_step_table(timesteps, positions, [flags[lay.request_of_row(b)] for b in range(B)])
                soft = dict(release=rel, table=torch.tensor(table, dtype=torch.int32).to(dev),
                            step_dev=torch.full((B,), -1, dtype=torch.int32, device=dev))          # the captured step reads its steps here
        keep_in = None if control is None else control.get("keep", [1.0] * len(timesteps))
        # (PNDM calls the UNet once more than it has steps: the extra call keeps the last gate)
        keeps = None if control is None else [keep_in[min(i, len(keep_in) - 1) if fused else i] for i in range(len(timesteps))]
        noisy = fused and sch.stochastic                          # Euler-ancestral: noise every step, whatever eta
        stochastic = (float(eta) > 0.0 and not multistep and not fused) or noisy
        if variance_noise is not None and stochastic and len(variance_noise) < len(timesteps):
            raise ValueError(f"variance_noise has {len(variance_noise)} entries for {len(timesteps)} steps")
        ctrl_scale = 0.0 if control is None else float(control.get("scale", 1.0))
        # control["rows"] (enable_request_control_scales, the triples differ): the rows route for the whole call -- the effective scale of
        # every batch row at every UNet call, uploaded once; the captured step of a graph reads the fixed-address ctrl_dev instead
        ctrl_table = ctrl_dev = None
        if control is not None and control.get("rows") is not None:
            if len(control["rows"]) != lay.requests:
                raise ValueError(f"control rows: {len(control['rows'])} requests' scales for {lay.requests} requests")
            ctrl_table = control_scale_table(control["rows"], len(timesteps), lay, clamp=fused).to(dev)
            ctrl_dev = torch.ones(2 * B, dtype=torch.float32, device=dev)
        # several nets: ONE table [calls, K, 2B] for the whole call, uploaded once; ctrl_run[i][k]: does net k contribute to any row at
        # call i?  The eager loop does not run a net that does not (its source is at scale 0 in the mix launch, which never reads it)
        ctrl_run = None
        control_net = self._single_controlnet()
        if multi:
            nets = self._control_nets()
            if len(control["multi_rows"]) != len(nets) or len(ctrl_img) != len(nets):
                raise ValueError(f"control: {len(control['multi_rows'])} nets' scales and {len(ctrl_img)} images for {len(nets)} ControlNets")
            if any(len(r) != lay.requests for r in control["multi_rows"]):
                raise ValueError(f"control multi_rows: every net needs the scales of {lay.requests} requests")
            host_table = multi_control_scale_table(control["multi_rows"], len(timesteps), lay, clamp=fused)
            ctrl_run = [[bool(host_table[i, k].ne(0).any()) for k in range(len(nets))] for i in range(len(timesteps))]
            ctrl_table = host_table.to(dev)
            ctrl_dev = torch.zeros(len(nets), 2 * B, dtype=torch.float32, device=dev)

        def control_residuals(t, i, mode):
            """the ControlNet forward of UNet call ``i`` (None: the captured step of a graph replay) -> (down, mid)"""
            if control is None:
                return None, None
            if multi:
                return self.controlnet.forward_nhwc(x_in, t, ctrl_ehs, ctrl_img, ctrl_dev if i is None else ctrl_table[i],
                                                    run=None if i is None else ctrl_run[i], **mode)
            if ctrl_table is not None:
                return control_net.forward_nhwc(x_in, t, ctrl_ehs, ctrl_img, 1.0, scale_rows=ctrl_dev if i is None else ctrl_table[i], **mode)
            return control_net.forward_nhwc(x_in, t, ctrl_ehs, ctrl_img, ctrl_scale * (keeps[0] if i is None else keeps[i]), **mode)
        # DeepCache (enable_deepcache): one feature cache for this call, shared by the UNet and the ControlNet; UNet call i == loop index i
        # (timesteps holds the executed calls only, PNDM's extra one included).  Switch off or interval 1: no cache, no keyword, today's calls
        dc_on = getattr(self, "_deepcache", None) is not None
        dc = DeepCache(self._deepcache[1]) if dc_on and self._deepcache[0] > 1 else None
        dc_plan = deepcache_plan(len(timesteps), self._deepcache[0]) if dc is not None else None

        def dc_kw(i):
            """the cache keyword of UNet (and ControlNet) call ``i``, in the mode the plan gives it"""
            if dc is None:
                return {}
            dc.full = dc_plan[i]
            return {"deepcache": dc}

        dev_noise = noise_plan is not None and stochastic and variance_noise is None
        if dev_noise:
            if noise_plan.rows != B or Cl != 4:
                raise ValueError(f"device noise: {noise_plan.rows} keyed rows for {B} latent rows of {Cl} channels")
            from ...noise import step_draws
            key_table = noise_plan.key_table(step_draws(t_start, len(timesteps)))
            key_dev = torch.zeros_like(key_table[0])          # the captured step reads its keys here
            noise_buf = torch.zeros(B, HW, Cl, dtype=torch.float32, device=dev)

        def step_noise(i):
            if dev_noise:          # (i is None: the captured step of a graph replay)
                return ops.noise_rows(noise_buf, key_dev if i is None else key_table[i])
            vn = variance_noise[i] if variance_noise is not None else randn_tensor((B, Cl, h, w), generator=generator, device=dev, dtype=dt)
            return vn.to(device=dev, dtype=torch.float32).permute(0, 2, 3, 1).reshape(B, HW, Cl).contiguous()

        if fused:
            # the history buffer [K][B HW 4] lives for the whole call at one address; which slot a step reads and writes is part of its
            # coefficient row (scheduler.SamplerHistory), so the rows of the whole run are known before the first launch
            from ...scheduler import SamplerHistory, UniPCHistory
            hist = torch.zeros(sch.history, B, HW, Cl, dtype=torch.float32, device=dev) if sch.history else None
            ring = UniPCHistory(sch.history) if unipc else SamplerHistory(sch.history)
            plan = sch.plan_fused if unipc else sch.plan          # (UniPC: 19 values per step, two store slots)
            sampler_rows = [ring.coefs(plan(i, int(t_start), blend=inp is not None)) for i in range(len(timesteps))]

        def sampler_step(t, i=None, coefs=None):
            """ControlNet + UNet + ONE imd_sampler_step -- imd_unipc_step for UniPC -- (CFG / update / history / noise / blend / next UNet input); ``t``, ``coefs`` as
            for ``ddim_step`` (graph replay: the coefficient row, history slot included, is read from device memory)."""
            mode = {} if i is None else dc_kw(i)          # (i is None: the captured step of a graph replay, which never runs with the cache)
            down, mid = control_residuals(t, i, mode)
            eps = self.unet.forward_nhwc(x_in, t, ehs, cak, down, mid, cfg_pair=True, **mode)
            if phi_arg is not None:
                ops.guidance_rescale(eps.view(2 * B, HW, Cl), guidance=g_arg, rescale=phi_arg)
            kw = {}
            if inp is not None:
                kw = dict(mask=inp["mask"], z_img=inp["z_img"], blend_noise=inp["noise"])
            if noisy:
                kw["noise"] = step_noise(i)
            if soft is not None:
                ops.soft_mask_rows(inp["mask"], soft["release"], soft["step_dev"] if i is None else soft["table"][i])
            (ops.unipc_step if unipc else ops.sampler_step)(z, eps, x_in.view(2 * B, HW, 8), guidance=g_arg, coefs=sampler_rows[i] if coefs is None else coefs, hist=hist, **kw)

        def ddim_step(t, i=None, coefs=None):
            """ControlNet + UNet + CFG / DDIM / blend / next UNet input for one timestep; ``t`` a Python int (eager) or a device
            scalar with ``coefs`` the device-side schedule coefficients (graph replay: nothing step-specific is baked in)."""
            mode = {} if i is None else dc_kw(i)
            down, mid = control_residuals(t, i, mode)
            eps = self.unet.forward_nhwc(x_in, t, ehs, cak, down, mid, cfg_pair=True, **mode)     # x_in = [z; z]: both halves see the same latent
            if phi_arg is not None:
                ops.guidance_rescale(eps.view(2 * B, HW, Cl), guidance=g_arg, rescale=phi_arg)
            kw = {}
            if inp is not None:
                kw = dict(mask=inp["mask"], z_img=inp["z_img"], noise=inp["noise"])
            if soft is not None:
                ops.soft_mask_rows(inp["mask"], soft["release"], soft["step_dev"] if i is None else soft["table"][i])
            if coefs is not None:
                ops.ddim_cfg_step(z, eps, x_in.view(2 * B, HW, 8), guidance=g_arg, coefs=coefs, **kw)
            else:
                if inp is not None:
                    kw["a_next"] = sch.alpha(timesteps[i + 1]) if i < len(timesteps) - 1 else None
                if stochastic:
                    kw["var_noise"] = step_noise(i)
                    kw["sigma"] = sch.sigma(timesteps[i], eta)
                ops.ddim_cfg_step(z, eps, x_in.view(2 * B, HW, 8), guidance=g_arg, a_t=sch.alpha(timesteps[i]),
                                  a_prev=sch.alpha_prev(timesteps[i]), **kw)

        # The time-embedding chain depends on the timestep only: one pass over the whole schedule here, every forward of the loop picks its row
        # (unet._Encoder.precompute_time_embeddings; 7 launches per UNet / ControlNet forward gone)
        encs = [m for m in [self.unet] + (self._control_nets() if control is not None else []) if hasattr(m, "precompute_time_embeddings")]
        tables = [e.precompute_time_embeddings(timesteps, dev) for e in encs] if ops.TEMB_TABLE else []
        if not tables:
            encs = []

        one_step = sampler_step if fused else ddim_step

        def run_steps():
            nonlocal z
            # (a stochastic step replays only where its noise is made on the device: Euler-ancestral with enable_device_noise)
            use_graph = (getattr(self, "_step_graph", False) and not dc_on and not multistep and (not stochastic or (noisy and dev_noise))
                         and callback is None and trace is None
                         and len(timesteps) > 2 and (keeps is None or ctrl_table is not None or len(set(keeps)) == 1) and ops.ATTN_EVENT_HOOK is None)
            if use_graph:
                # HIP-graph replay of the denoising step (opt-in, ``enable_step_graph``): step 0 runs eagerly on the pipeline's side stream
                # (it also fills the step-invariant K / V caches of the processors), step 1 is CAPTURED (not executed) into a graph whose
                # only per-step inputs are two device scalars -- the timestep and the six schedule coefficients -- and the graph is then
                # replayed for steps 1 .. S-1: ~500 kernel launches per step become one hipGraphLaunch (the loop is host-bound at batch 1).
                steps_n = len(timesteps)
                t_table = torch.tensor(timesteps, dtype=torch.float32).to(dev)
                rows = sampler_rows if fused else []          # (fused samplers: 13 values per step -- UniPC: 19 --, history slots included)
                if not fused:
                    for i, t in enumerate(timesteps):
                        a_next = (sch.alpha(timesteps[i + 1]) if i < steps_n - 1 else None) if inp is not None else None
                        rows.append(ops.ddim_coefs(sch.alpha(t), sch.alpha_prev(t), a_next))
                coef_table = torch.tensor(rows, dtype=torch.float32).to(dev)
                t_dev = torch.zeros(1, dtype=torch.float32, device=dev)
                coef_dev = torch.zeros(coef_table.shape[1], dtype=torch.float32, device=dev)
                side = self.__dict__.get("_graph_stream")
                if side is None:
                    side = self._graph_stream = torch.cuda.Stream(device=dev)
                cur = torch.cuda.current_stream(dev)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    t_dev.copy_(t_table[0:1]); coef_dev.copy_(coef_table[0])
                    if dev_noise:
                        key_dev.copy_(key_table[0])
                    if ctrl_table is not None:
                        ctrl_dev.copy_(ctrl_table[0])
                    if soft is not None:
                        soft["step_dev"].copy_(soft["table"][0])
                    temb_bufs = [torch.empty_like(tab[0:1]) for tab in tables]     # fixed addresses inside the captured step, refreshed like t_dev
                    for e, buf, tab in zip(encs, temb_bufs, tables):
                        buf.copy_(tab[0:1])
                        e.use_time_embedding(buf)
                    one_step(t_dev, coefs=coef_dev)
                    g = torch.cuda.CUDAGraph()
                    g.capture_begin()
                    try:
                        one_step(t_dev, coefs=coef_dev)
                    finally:
                        g.capture_end()
                    for i in range(1, steps_n):
                        t_dev.copy_(t_table[i:i + 1]); coef_dev.copy_(coef_table[i])
                        if dev_noise:
                            key_dev.copy_(key_table[i])
                        if ctrl_table is not None:
                            ctrl_dev.copy_(ctrl_table[i])
                        if soft is not None:
                            soft["step_dev"].copy_(soft["table"][i])
                        for buf, tab in zip(temb_bufs, tables):
                            buf.copy_(tab[i:i + 1])
                        g.replay()
                cur.wait_stream(side)
                self._last_step_graph = g          # keep the executable graph alive until the next call (replays may still be in flight)
                return z.view(B, h, w, Cl).permute(0, 3, 1, 2).contiguous()
            for i, t in enumerate(timesteps):
                if multistep:
                    mode = dc_kw(i)
                    down, mid = control_residuals(t, i, mode)
                    eps = self.unet.forward_nhwc(x_in, t, ehs, cak, down, mid, cfg_pair=True, **mode)
                    z = sch.step_guided(eps.view(2 * B, HW, Cl), z, gs[0])
                    # emit the next 16-bit UNet input (both CFG halves) from z: the fused step with eps = 0, alpha = 1 is the identity on z
                    ops.ddim_cfg_step(z, ops.workspace("zero_eps", (2 * B, HW, Cl), torch.float32, dev), x_in.view(2 * B, HW, 8),
                                      guidance=1.0, a_t=1.0, a_prev=1.0)
                else:
                    one_step(t, i)
                if trace is not None:
                    trace.append(z.clone())
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, z.view(B, h, w, Cl).permute(0, 3, 1, 2))
            return z.view(B, h, w, Cl).permute(0, 3, 1, 2).contiguous()

        try:
            return run_steps()
        finally:
            for e in encs:
                e.clear_time_embeddings()
            if dc is not None:
                dc.clear()          # the stored feature dies with the call, an exception included

    # ---- in-flight batching (imagdressing_amd/session.py) ----
    def _open_session(self, slots: int, width: int, height: int, controlnet_conditioning_scale: float = 1.0, with_controlnet: bool = False,
                      compact: bool = False, widths=None, device_noise: Optional[bool] = None, control_rows: Optional[bool] = None):
        """A denoising session of ``slots`` latent rows at one geometry: requests are submitted at any time, enter a free slot at the
        start of any step, run their own number of steps and leave when done (``session.DenoiseSession``).  DPM-Solver++, Euler, PNDM
        and DDIM (eta = 0), UniPC after ``scheduler.enable_fused_step()``; refused with UniPC otherwise, Euler-ancestral and while ``enable_deepcache`` is on; ``enable_step_graph`` is ignored.
        ``compact=True``: every step runs a batch only as wide as the running requests need -- the smallest entry of ``widths`` (None:
        every width 1..slots; else a strictly increasing tuple that ends at ``slots``) -- and a request's bits then depend on the
        widths it ran under.
        ``device_noise`` (None: follow ``enable_device_noise``): every request carries a seed (``submit(seed=...)``) and its noise is
        made on the device, one ``imd_noise_rows`` launch per step for all slots -- Euler-ancestral is then accepted, and so is
        ``submit(eta=...)`` > 0 under DDIM, per request; a request's latents do not depend on its slot or on the other requests.
        ``control_rows`` (None: follow ``enable_request_control_scales``; a session with a ControlNet only): the ControlNet scale and
        its guidance window are per request -- ``submit(controlnet_conditioning_scale=, control_guidance_start=, control_guidance_end=)``
        -- and EVERY step takes the rows route (``imd_residual_scale_rows`` behind the ControlNet at ``out_scale`` 1), so that a request's
        bits cannot depend on whether its company happens to share its values."""
        from ...session import DenoiseSession
        self._refuse_multi("open_session")
        return DenoiseSession(self, slots, width, height, controlnet_conditioning_scale, with_controlnet=with_controlnet, compact=compact,
                              widths=widths, device_noise=device_noise, control_rows=control_rows)

    # ---- request-batched calls (RequestLayout) ----
    def _request_count(self, args: Dict[str, Any], per_call: Dict[str, Any], shard_over_ranks: bool,
                       control: Optional[Dict[str, Any]] = None) -> int:
        """``control``: the ControlNet pipelines' ``controlnet_conditioning_scale`` / ``control_guidance_start`` / ``control_guidance_end``.
        Switch off (``enable_request_control_scales``): they are checked as ever -- the scale per call, the window not at all."""
        if control is not None and getattr(self, "_request_control_scales", False):
            per_call = {k: v for k, v in per_call.items() if k not in CONTROL_KEYS}
            return request_count(args, per_call, shard_over_ranks=shard_over_ranks, scheduler=self.scheduler, control=control)
        return request_count(args, per_call, shard_over_ranks=shard_over_ranks, scheduler=self.scheduler)

    def _request_prompts(self, R, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, device, clip_skip=None):
        """(prompt embeds, negative embeds): [1 | R, T, C] each -- R rows as soon as either side speaks per request"""
        pe, ne = self.encode_prompt(prompt, device, 1, True, negative_prompt, prompt_embeds=prompt_embeds,
                                    negative_prompt_embeds=negative_prompt_embeds, clip_skip=clip_skip)
        if R > 1:
            pe, ne = request_rows(pe, R, "prompt / prompt_embeds"), request_rows(ne, R, "negative_prompt / negative_prompt_embeds")
        return pe, ne

    def _request_garments(self, R, null_prompt, ref_image, ref_image_latents, ref_clip_image, ref_clip_hidden_states, device):
        """(garment latents, garment tokens, G): G = R distinct garments when a garment argument speaks per request, else 1 (one garment
        shared by every request, the single-request path)."""
        if ref_clip_image is None and ref_clip_hidden_states is None:
            # the reference falls back to text "null prompt" tokens as garment-UNet context (:416-427)
            cloth_tokens, _ = self.encode_prompt(null_prompt, device, 1, False)
        else:
            cloth_tokens = self._cloth_tokens(as_batch(ref_clip_image, "ref_clip_image"), ref_clip_hidden_states, device)      # :409-415
        ref_lat = self._ref_latents(as_batch(ref_image, "ref_image"), ref_image_latents)                                     # :454-458
        if R > 1 and (ref_lat.shape[0] == R or cloth_tokens.shape[0] == R):
            return request_rows(ref_lat, R, "ref_image / ref_image_latents"), request_rows(cloth_tokens, R, "garment tokens"), R
        return ref_lat, cloth_tokens, 1

    @staticmethod
    def _image_scales(image_scale, R):
        """-> (the scale the processors get through set_scale, per-request weights for the loop or None).  Equal values (and a scalar) keep
        the reference's set_scale behaviour; differing ones ride in the sa_batch_mask rows with the processors' scale at 1."""
        if not _is_seq(image_scale):
            return image_scale, None
        vals = per_request_floats("image_scale", image_scale, R)
        return (vals[0], None) if len(set(vals)) == 1 else (1.0, vals)

    # ---- shared front / back end ----
    def _cloth_tokens(self, ref_clip_image, ref_clip_hidden_states, device):
        """(cloth_proj_embed, cloth_null_embeds) [1,16,768] each (:409-415).  The null tokens are computed for
        API parity only -- the garment UNet's null half is discarded by the reference (:476-480)."""
        if ref_clip_hidden_states is None:
            ref_clip_hidden_states = self._clip_hidden(ref_clip_image, device)
        return self.ImgProj(ref_clip_hidden_states.to(device))

    def _ref_latents(self, ref_image, ref_image_latents):
        if ref_image_latents is not None:
            return ref_image_latents
        p = next(self.vae.parameters())
        return self.vae.encode(ref_image.to(dtype=p.dtype, device=p.device)).latent_dist.mean * 0.18215   # :457-458

    def _decode_nhwc(self, latents) -> list:
        """final latents -> the decoder's 16-bit NHWC output, one tensor (or one per image: VAE slicing) -- the device image route"""
        p = next(self.vae.parameters())
        z = (latents / self.vae.config.scaling_factor).to(p.dtype)
        ops.ensure_device(z.device)
        slices = z.split(1) if getattr(self.vae, "use_slicing", False) and z.shape[0] > 1 else (z,)
        return [self.vae.decode_nhwc(nchw_to_nhwc8(zb.float(), self.vae.dtype)) for zb in slices]       # (AutoencoderKL.decode, without its NCHW copy)

    def _decode(self, latents, output_type, generator=None):
        if output_type == "latent":
            return StableDiffusionPipelineOutput(images=latents, nsfw_content_detected=None)
        p = next(self.vae.parameters())
        if getattr(self, "_device_image_io", False) and output_type in ("np", "pil"):
            if not hasattr(self.vae, "decode_nhwc"):
                raise TypeError("enable_device_image_io() needs the engine VAE (imagdressing_amd.vae.AutoencoderKL.decode_nhwc), got "
                                f"{type(self.vae).__module__}.{type(self.vae).__name__}")
            ys = self._decode_nhwc(latents)
            return StableDiffusionPipelineOutput(images=self._image_processor().postprocess(ys, output_type), nsfw_content_detected=None)
        image = self.vae.decode((latents / self.vae.config.scaling_factor).to(p.dtype), return_dict=False)[0]
        image = (image.float() / 2 + 0.5).clamp(0, 1)
        if output_type == "pt":
            return StableDiffusionPipelineOutput(images=image, nsfw_content_detected=None)
        arr = (image.permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8")
        if output_type == "np":
            return StableDiffusionPipelineOutput(images=arr, nsfw_content_detected=None)
        from PIL import Image
        return StableDiffusionPipelineOutput(images=[Image.fromarray(a) for a in arr], nsfw_content_detected=None)

    def _shard(self, latents, shard: bool):
        """Data-parallel sharding of the image batch over torch.distributed ranks (no-op single process)."""
        from ... import dist as imd_dist
        return imd_dist.shard_rows(latents) if shard else latents

    def _sa_states(self, ref_latents, cloth_tokens, shard: bool, garments: int = 1):
        from ... import dist as imd_dist
        if garments > 1:          # (request-batched calls refuse shard_over_ranks up front: request_count)
            return self.garment_features(ref_latents, cloth_tokens, garments)
        if shard and imd_dist.world_size() > 1:
            return imd_dist.garment_features_broadcast(self, ref_latents, cloth_tokens)
        return self.garment_features(ref_latents, cloth_tokens)


# ---- request-batched calls: R distinct (garment, prompt, pose / mask / face) requests in one pipeline call ----
@dataclass(frozen=True)
class RequestLayout:
    """Row layout of a call with ``requests`` = R requests of ``images_per_request`` = n images each.

    Latent rows are request-major: request r owns rows [r n, (r+1) n).  The UNet runs the CFG batch of 2 R n rows -- [0, Rn) cond,
    [Rn, 2Rn) uncond -- against the text context [R prompts; R negatives] (``text_context``): the processors' kv batch divisor
    (rows / context rows = n) maps UNet row b to context row :meth:`ehs_row`.  Garment tensors [R, M, C] serve the cond rows
    (``sa_pair_layout``): cond row b reads garment :meth:`garment_of_row`; uncond rows have no garment branch.  R = 1 is today's
    single-request layout: context [prompt, negative], one garment."""
    requests: int
    images_per_request: int

    @property
    def rows(self) -> int:
        return self.requests * self.images_per_request

    def request_of_row(self, b: int) -> int:
        """request of latent row b (= of cond row b and of uncond row rows + b)"""
        return (b % self.rows) // self.images_per_request

    def ehs_row(self, b: int) -> int:
        """text-context row of UNet row b of the CFG batch"""
        return b // self.images_per_request

    def garment_of_row(self, b: int) -> Optional[int]:
        """garment of UNet row b (None: an uncond row, garment branch off)"""
        return b // self.images_per_request if b < self.rows else None

    def per_row(self, values: Sequence[float]) -> torch.Tensor:
        """R per-request values -> [rows] fp32, one per latent row"""
        return torch.tensor([float(v) for v in values], dtype=torch.float32).repeat_interleave(self.images_per_request)

    def expand(self, t: torch.Tensor, name: str) -> torch.Tensor:
        """[1 | R | rows, ...] -> [rows, ...] (request-major)"""
        if t.shape[0] == self.rows:
            return t
        if t.shape[0] == 1:
            return t.expand(self.rows, *t.shape[1:])
        if t.shape[0] == self.requests:
            return t.repeat_interleave(self.images_per_request, 0)
        raise ValueError(f"{name} has {t.shape[0]} rows; expected 1, {self.requests} (one per request) or {self.rows} (one per image)")

    def text_context(self, prompt_embeds: torch.Tensor, negative_prompt_embeds: torch.Tensor) -> torch.Tensor:
        """[prompts; negatives]: [2, T, C] for one request (row 0 of each, as the single-request loop always took), [2R, T, C] otherwise"""
        if self.requests == 1:
            return torch.cat([prompt_embeds[:1], negative_prompt_embeds[:1]])
        return torch.cat([request_rows(prompt_embeds, self.requests, "prompt_embeds"),
                          request_rows(negative_prompt_embeds, self.requests, "negative_prompt_embeds")])


def request_rows(t: torch.Tensor, R: int, name: str) -> torch.Tensor:
    """[1 | R, ...] -> [R, ...]: one shared entry or one per request"""
    if t.shape[0] == R:
        return t
    if t.shape[0] == 1:
        return t.expand(R, *t.shape[1:])
    raise ValueError(f"{name} has {t.shape[0]} entries for {R} requests (give one, shared, or one per request)")


def _is_seq(v) -> bool:
    return isinstance(v, (list, tuple))


def per_request_floats(name: str, value, R: int) -> List[float]:
    """a float or a sequence of 1 or R floats -> R floats"""
    vals = [float(v) for v in value] if _is_seq(value) else [float(value)]
    if len(vals) == 1:
        return vals * R
    if len(vals) != R:
        raise ValueError(f"{name} has {len(vals)} entries for {R} requests")
    return vals


def guidance_rescale_values(value, R: int) -> List[float]:
    """``guidance_rescale`` of a call or a session request -> R floats, each finite and in [0, 1] (diffusers takes any float; outside
    [0, 1] the factor extrapolates past both standard deviations, which no caller means)"""
    vals = per_request_floats("guidance_rescale", value, R)
    for v in vals:
        if not (math.isfinite(v) and 0.0 <= v <= 1.0):
            raise ValueError(f"guidance_rescale must be finite and in [0, 1], got {v}")
    return vals


def soft_step_table(timesteps: Sequence, positions: int, soft_rows: Sequence[bool]) -> List[List[int]]:
    """``soft_mask``: the step k of every UNet call of a run, per latent row -- [calls][B], -1 for a hard row.  ``timesteps``: the
    executed calls; call i blends towards ``timesteps[i + 1]`` (the last call: towards the clean image latents), and k counts the
    distinct positions aimed at so far, so PNDM's doubled first call holds k = 0 twice; ``positions`` = n caps k at n - 1, the blend
    of the last position.  DDIM, DPM-Solver++, Euler and UniPC: k = i.  PNDM at ``strength`` < 1 from schedule position 2 or later is
    the one case in which ``positions`` is FEWER than the distinct positions aimed at: the slice of its doubled timestep list then
    holds no doubled entry, its n + 1 calls aim at n + 1 levels, and the table ends [.., n - 1, n - 1] -- the cap keeps a pixel whose
    release is n the clean original."""
    ks, k = [], 0
    for i in range(len(timesteps)):
        aim = timesteps[i + 1] if i + 1 < len(timesteps) else None
        if i > 0 and aim != timesteps[i]:          # (timesteps[i] is what call i - 1 aimed at)
            k += 1
        ks.append(min(k, int(positions) - 1))
    return [[k if s else -1 for s in soft_rows] for k in ks]


def per_call_value(name: str, value):
    """Arguments folded into weights or shared by the schedule (steps, strength, eta, LoRA / IP-Adapter / ControlNet scales) stay per call:
    a sequence is accepted only if its entries agree."""
    if not _is_seq(value):
        return value
    if len(value) == 0 or any(v != value[0] for v in value):
        raise ValueError(f"{name} is per call (it is folded into weights or shared by the schedule), got differing values {list(value)}")
    return value[0]


# batched rank of the tensor form of each per-request argument (a tensor of lower rank is ONE entry)
_BATCHED_NDIM = dict(ref_image=4, ref_clip_image=4, ref_clip_hidden_states=3, ref_image_latents=4, prompt_embeds=3, negative_prompt_embeds=3,
                     control_image=4, pose_image=4, image=4, mask_image=4, image_latents=4, mask_latents=4, face_clip_image=4, faceid_embeds=2,
                     face_clip_hidden_states=3, face_uncond_clip_hidden_states=3)


def entries(name: str, value) -> Optional[int]:
    """How many requests an argument speaks for: a list's length, a tensor's / array's batch, None for a single value (str, float, image)."""
    if value is None or isinstance(value, (str, bytes, int, float)):
        return None
    if _is_seq(value):
        return len(value)
    shape = getattr(value, "shape", None)
    if shape is not None and len(shape) == _BATCHED_NDIM.get(name, -1):
        return int(shape[0])
    return None


# the arguments R is inferred from (garment and prompt)
REQUEST_KEYS = ("prompt", "prompt_embeds", "ref_image", "ref_clip_image", "ref_clip_hidden_states", "ref_image_latents")
PER_CALL_KEYS = ("num_inference_steps", "strength", "eta", "ipa_scale", "s_lora_scale", "c_lora_scale", "controlnet_conditioning_scale")


CONTROL_KEYS = ("controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end")


def control_request_values(scale, start, end, R: int) -> List[tuple]:
    """The three ControlNet arguments of a call with ``enable_request_control_scales`` -> R triples (scale, start, end).  Each is one
    value or a sequence of 1 or R (else ValueError naming it).  Where any of them is a sequence: every scale is finite and every
    window satisfies 0 <= start < end <= 1 (the rule of diffusers' ``check_inputs``); scalars are taken as they are, like the switch-off
    path takes them."""
    cols = [per_request_floats(k, v, R) for k, v in zip(CONTROL_KEYS, (scale, start, end))]
    triples = list(zip(*cols))
    if any(_is_seq(v) for v in (scale, start, end)):
        for r, (s, a, b) in enumerate(triples):
            if not math.isfinite(s):
                raise ValueError(f"controlnet_conditioning_scale of request {r} must be finite, got {s}")
            if not (math.isfinite(a) and math.isfinite(b) and 0.0 <= a < b <= 1.0):
                raise ValueError(f"control_guidance_start / control_guidance_end of request {r}: need 0 <= start < end <= 1, got "
                                 f"start = {a}, end = {b}")
    return triples


def control_plan(scale, start, end, R: int, steps: int, *, per_request: bool = False):
    """-> (scale, keep, rows) for the ``control`` dict of :meth:`PipelineBase._denoise`.  ``per_request`` False (the switch is off),
    or the R triples agree: the FOLDED route -- the first entries as ever, ``rows`` None.  Otherwise the ROWS route for the whole call:
    scale 1.0, keep all 1 and ``rows[r][i] = scale_r * controlnet_keep(steps, start_r, end_r)[i]``, the effective scale of request r at
    loop index i."""
    if per_request:
        triples = control_request_values(scale, start, end, R)
        if len(set(triples)) > 1:
            rows = [[s * k for k in controlnet_keep(steps, a, b)] for s, a, b in triples]
            return 1.0, [1.0] * steps, rows
        scale, start, end = triples[0]
    return float(first(scale)), controlnet_keep(steps, float(first(start)), float(first(end))), None


def control_scale_table(rows: Sequence[Sequence[float]], calls: int, lay: "RequestLayout", clamp: bool) -> torch.Tensor:
    """``rows`` of :func:`control_plan` -> the host table [calls, 2 lay.rows] fp32 that ``imd_residual_scale_rows`` reads one row of per
    UNet call: request-major over the images of a request (``RequestLayout.per_row``), the cond half then the same values for the
    uncond half.  ``clamp``: a call index past the gate's length reads its last entry (PNDM calls the UNet once more than it has
    steps)."""
    n = len(rows[0])
    if not clamp and calls > n:
        raise ValueError(f"the ControlNet gate has {n} entries for {calls} UNet calls")
    return torch.stack([lay.per_row([r[min(i, n - 1)] for r in rows]).repeat(2) for i in range(calls)])


def multi_control_values(scale, start, end, K: int, R: int, *, per_request: bool = False) -> List[List[tuple]]:
    """The three ControlNet arguments of a call on K >= 2 nets -> ``values[k][r]`` = (scale, start, end) of net k for request r.  Each
    argument is one value (all nets) or a flat list of K (per net: the diffusers meaning); with ``per_request``
    (``enable_request_control_scales``) each of the K entries may itself be a list of 1 or R values.  A wrong length raises ValueError
    naming the argument and both counts.  Every scale is finite and every window satisfies 0 <= start < end <= 1."""
    cols = []
    for name, v in zip(CONTROL_KEYS, (scale, start, end)):
        if _is_seq(v):
            if len(v) != K:
                raise ValueError(f"{name} has {len(v)} entries for {K} ControlNets (give one value for all nets, or one per net)")
            per_net = list(v)
        else:
            per_net = [v] * K
        col = []
        for k, e in enumerate(per_net):
            if _is_seq(e):
                if not per_request:
                    raise ValueError(f"{name}[{k}] is a list: a value per request needs enable_request_control_scales() (one value per "
                                     f"net otherwise)")
                if len(e) not in (1, R):
                    raise ValueError(f"{name}[{k}] has {len(e)} entries for {R} requests (give one, shared, or one per request)")
                col.append([float(x) for x in e] * (R if len(e) == 1 else 1))
            else:
                col.append([float(e)] * R)
        cols.append(col)
    values = [[(cols[0][k][r], cols[1][k][r], cols[2][k][r]) for r in range(R)] for k in range(K)]
    for k, per_req in enumerate(values):
        for r, (s, a, b) in enumerate(per_req):
            if not math.isfinite(s):
                raise ValueError(f"controlnet_conditioning_scale of net {k}, request {r} must be finite, got {s}")
            if not (math.isfinite(a) and math.isfinite(b) and 0.0 <= a < b <= 1.0):
                raise ValueError(f"control_guidance_start / control_guidance_end of net {k}, request {r}: need 0 <= start < end <= 1, got "
                                 f"start = {a}, end = {b}")
    return values


def multi_control_plan(scale, start, end, K: int, R: int, steps: int, *, per_request: bool = False) -> List[List[List[float]]]:
    """-> ``rows[k][r][i] = scale * controlnet_keep(steps, start, end)[i]`` of net k for request r (:func:`multi_control_values`): the
    effective scale at loop index i.  A call on K >= 2 nets always takes this route, whatever the values."""
    return [[[s * g for g in controlnet_keep(steps, a, b)] for s, a, b in per_req]
            for per_req in multi_control_values(scale, start, end, K, R, per_request=per_request)]


def multi_control_scale_table(rows: Sequence[Sequence[Sequence[float]]], calls: int, lay: "RequestLayout", clamp: bool) -> torch.Tensor:
    """``rows`` of :func:`multi_control_plan` -> the host table [calls, K, 2 lay.rows] fp32 that ``imd_residual_mix_rows`` reads one
    [K, 2B] slice of per UNet call: :func:`control_scale_table` per net (the cond half, then the same values for the uncond half;
    ``clamp``: PNDM's extra call reads the last gate)."""
    return torch.stack([control_scale_table(r, calls, lay, clamp) for r in rows], dim=1).contiguous()


def multi_control_images(name: str, images, K: int, R: int, allow_none: int = 0) -> list:
    """The control image argument of a call on K >= 2 nets: a list of K entries, one per net, each whatever one net takes (one image,
    or a per-request list / batched tensor of 1 or R); at most ``allow_none`` of them None."""
    if not _is_seq(images) or len(images) != K:
        n = len(images) if _is_seq(images) else (0 if images is None else 1)
        raise ValueError(f"{name} has {n} entries for {K} ControlNets (give a list with one entry per net)")
    if sum(e is None for e in images) > allow_none:
        raise ValueError(f"{name}: {sum(e is None for e in images)} of the {K} entries are None (at most {allow_none} may be)")
    for k, e in enumerate(images):
        c = entries(name, e)
        if c is not None and c not in (1, R):
            raise ValueError(f"{name}[{k}] has {c} entries for {R} requests (give one, shared, or one per request)")
    return list(images)


def request_count(args: Dict[str, Any], per_call: Optional[Dict[str, Any]] = None, *, shard_over_ranks: bool = False,
                  scheduler=None, control: Optional[Dict[str, Any]] = None) -> int:
    """R of a call and the checks of a request-batched one.  R = the largest entry count of the garment / prompt arguments
    (``REQUEST_KEYS``; 1 when all are single).  Every per-request argument in ``args`` has 1 entry (shared) or R, else ValueError
    naming it; the per-call arguments in ``per_call`` must not differ; ``shard_over_ranks`` and UniPC with differing guidance raise.
    ``control`` (``enable_request_control_scales``): the three ``CONTROL_KEYS`` arguments, per request -- :func:`control_request_values`."""
    counts = {k: entries(k, v) for k, v in args.items()}
    R = max([c for k, c in counts.items() if k in REQUEST_KEYS and c is not None] or [1])
    for k, c in counts.items():
        if c is not None and c not in (1, R):
            raise ValueError(f"{k} has {c} entries for {R} requests (give one, shared, or one per request)")
    if control is not None:
        control_request_values(*(control.get(k, d) for k, d in zip(CONTROL_KEYS, (1.0, 0.0, 1.0))), R)
    if R > 1:
        for k, v in (per_call or {}).items():
            per_call_value(k, v)
        if shard_over_ranks:
            raise NotImplementedError("shard_over_ranks with several requests in one call: sharding requests over ranks needs a garment "
                                      "UNet per rank (dist.garment_features_broadcast serves one garment); call per request instead")
    g = args.get("guidance_scale")
    if g is not None and _is_seq(g):
        gs = per_request_floats("guidance_scale", g, R)
        if scheduler is not None and hasattr(scheduler, "step_guided") and not unipc_fused(scheduler) and len(set(gs)) > 1:
            raise ValueError("guidance_scale differs between the requests: UniPC takes one guidance scale per call (the per-request "
                             "guidance step is the fused DDIM step)")
    if "image_scale" in args and _is_seq(args["image_scale"]):
        per_request_floats("image_scale", args["image_scale"], R)
    if "guidance_rescale" in args:
        guidance_rescale_values(args["guidance_rescale"], R)
    return R


def as_batch(value, name: str):
    """A per-request image argument as ONE batched tensor: a list of tensors is concatenated ([C, H, W] entries get a batch axis);
    anything else (a tensor, a PIL image or a list of them, None) is returned as is."""
    if _is_seq(value) and value and all(isinstance(v, torch.Tensor) for v in value):
        return torch.cat([v if v.dim() == _BATCHED_NDIM.get(name, v.dim()) else v.unsqueeze(0) for v in value])
    return value


def min_guidance(guidance_scale) -> float:
    return min(float(v) for v in guidance_scale) if _is_seq(guidance_scale) else float(guidance_scale)


def controlnet_keep(num_steps: int, start: float, end: float) -> List[float]:
    """diffusers' per-step ControlNet gate (..._pipeline_ipa_controlnet.py:582-590)."""
    return [1.0 - float(i / num_steps < start or (i + 1) / num_steps > end) for i in range(num_steps)]


def first(x):
    return x[0] if isinstance(x, (list, tuple)) else x


def to_image_tensor(image, device, normalize: bool, size=None, multiple: int = 8) -> torch.Tensor:
    """PIL / ndarray / tensor -> [B, 3, H, W] float in [0, 1] (or [-1, 1] when ``normalize``).

    ``size`` = (height, width) requested by the caller: like diffusers' ``prepare_image`` /
    ``VaeImageProcessor.preprocess`` (call sites ..._controlnet.py:480-501, ..._inpainting.py:352-369) the image is resized
    to it, rounded DOWN to a multiple of ``multiple`` (the VAE scale factor) -- PIL inputs with PIL's Lanczos filter (the
    processor's default ``resample``), tensors / arrays with ``F.interpolate``'s default (nearest), as the library does.
    The pipelines then read the output size back from this tensor (:501), so it always divides by 8."""
    import numpy as np
    hw = None
    if size is not None:
        hw = (int(size[0]) // multiple * multiple, int(size[1]) // multiple * multiple)
    if isinstance(image, torch.Tensor):
        t = image.float()
        if t.dim() == 3:
            t = t.unsqueeze(0)
    else:
        if not isinstance(image, (list, tuple)):
            image = [image]
        ims = []
        for im in image:
            if hasattr(im, "convert"):
                im = im.convert("RGB")
                if hw is not None and (im.height, im.width) != hw:
                    from PIL import Image
                    im = im.resize((hw[1], hw[0]), resample=Image.LANCZOS)
            ims.append(np.asarray(im, dtype=np.float32) / 255.0)
        t = torch.from_numpy(np.stack(ims)).permute(0, 3, 1, 2)
        if normalize:
            t = t * 2.0 - 1.0
    if hw is not None and tuple(t.shape[-2:]) != hw:
        t = torch.nn.functional.interpolate(t, size=hw)
    return t.to(device)


def set_scale_by_type(unet, cls, **attrs):
    for proc in unet.attn_processors.values():
        if isinstance(proc, cls):
            for k, v in attrs.items():
                setattr(proc, k, v)


__all__ = ["deepcache_plan", "RequestLayout", "request_count", "request_rows", "unipc_fused", "per_request_floats", "guidance_rescale_values", "soft_step_table", "per_call_value", "as_batch", "min_guidance", "entries",
           "controlnet_keep", "control_plan", "control_request_values", "control_scale_table", "multi_control_values", "multi_control_plan", "multi_control_scale_table", "multi_control_images", "CONTROL_KEYS", "first", "to_image_tensor", "PipelineBase", "StableDiffusionPipelineOutput", "randn_tensor", "set_scale_by_type",
           "RefSAttnProcessor2_0", "LoraRefSAttnProcessor2_0", "LoRAIPAttnProcessor2_0", "IPAttnProcessor2_0"]
