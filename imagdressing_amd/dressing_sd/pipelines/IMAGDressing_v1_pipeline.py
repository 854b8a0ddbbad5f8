"""Base pipeline: text + garment conditioning, no ControlNet
(mirrors /root/reference/dressing_sd/pipelines/IMAGDressing_v1_pipeline.py:18-40, 342-547)."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ._base import PipelineBase, RefSAttnProcessor2_0, StableDiffusionPipelineOutput, min_guidance, per_call_value, set_scale_by_type


class IMAGDressing_v1(PipelineBase):
    _optional_components: list = []

    def __init__(self, vae, reference_unet, unet, tokenizer, text_encoder, image_encoder, ImgProj, scheduler,
                 safety_checker=None, feature_extractor=None):
        self._init_common(vae=vae, reference_unet=reference_unet, unet=unet, tokenizer=tokenizer, text_encoder=text_encoder,
                          image_encoder=image_encoder, ImgProj=ImgProj, scheduler=scheduler, safety_checker=safety_checker,
                          feature_extractor=feature_extractor)

    def set_scale(self, scale):                                            # :342-345
        set_scale_by_type(self.unet, RefSAttnProcessor2_0, scale=scale)

    def open_session(self, slots: int, width: int, height: int, controlnet_conditioning_scale: float = 1.0, compact: bool = False, widths=None,
                     device_noise: Optional[bool] = None):
        """In-flight batching: a :class:`imagdressing_amd.session.DenoiseSession` with ``slots`` slots at ``width`` x ``height``
        (``controlnet_conditioning_scale`` is accepted for a uniform surface; this pipeline has no ControlNet).  ``compact`` / ``widths``:
        run only as many batch rows as requests are running; ``device_noise``: per-request seeded noise, None = follow
        ``enable_device_noise`` (``_open_session``)."""
        return self._open_session(slots, width, height, compact=compact, widths=widths, device_noise=device_noise)

    @torch.no_grad()
    def __call__(self, prompt, null_prompt, negative_prompt, ref_image, width, height, num_inference_steps, guidance_scale,
                 ref_clip_image=None, num_images_per_prompt=1, image_scale=1.0, num_samples=1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, clip_skip: Optional[int] = None, callback: Optional[Callable] = None,
                 callback_steps: Optional[int] = 1, prompt_embeds: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 # --- extensions: bypass the out-of-scope encoders / inject latents / shard over ranks ---
                 ref_clip_hidden_states: Optional[torch.Tensor] = None, ref_image_latents: Optional[torch.Tensor] = None,
                 latents: Optional[torch.Tensor] = None, shard_over_ranks: bool = False, trace: Optional[list] = None,
                 guidance_rescale: Union[float, List[float]] = 0.0, **kwargs):
        R = self._request_count(dict(prompt=prompt, prompt_embeds=prompt_embeds, negative_prompt=negative_prompt, null_prompt=null_prompt,
                                     negative_prompt_embeds=negative_prompt_embeds, ref_image=ref_image, ref_clip_image=ref_clip_image,
                                     ref_clip_hidden_states=ref_clip_hidden_states, ref_image_latents=ref_image_latents,
                                     guidance_scale=guidance_scale, image_scale=image_scale, guidance_rescale=guidance_rescale),
                                dict(num_inference_steps=num_inference_steps, eta=eta), shard_over_ranks)
        num_inference_steps, eta = per_call_value("num_inference_steps", num_inference_steps), per_call_value("eta", eta)
        if min_guidance(guidance_scale) <= 1.0:
            # the reference cannot run this either: its loop indexes the CFG pair unconditionally (cache["hidden_states"][1] :476-479,
            # latent_model_input[1] :511) and null_prompt_embeds is only bound under do_classifier_free_guidance (:431-435)
            raise NotImplementedError("guidance_scale <= 1: the reference's loop indexes the CFG pair unconditionally "
                                      "(IMAGDressing_v1_pipeline.py:476-479, :511); sample with guidance_scale > 1")
        scale, scale_rows = self._image_scales(image_scale, R)
        self.set_scale(scale)                                              # :374
        device = self.device
        self._cross_attention_kwargs = cross_attention_kwargs
        prompt_embeds, negative_prompt_embeds = self._request_prompts(
            R, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, device, clip_skip)      # :395-405
        ref_lat, cloth_tokens, G = self._request_garments(R, null_prompt, ref_image, ref_image_latents, ref_clip_image,
                                                          ref_clip_hidden_states, device)              # :409-427, :454-458
        self.scheduler.set_timesteps(num_inference_steps, device=device)      # (init_noise_sigma may depend on the schedule; IMAGDressing_v1_pipeline.py:386)
        keyed = self._request_noise(kwargs, generator, R, num_images_per_prompt)          # enable_device_noise: seed= / generator -> one key per row
        lat = self.prepare_latents(R * num_images_per_prompt, 4, width, height, torch.float32, device, generator, latents, noise_plan=keyed)
        lat = self._shard(lat, shard_over_ranks)
        sa = self._sa_states(ref_lat, cloth_tokens, shard_over_ranks, G)                             # :465-480
        out = self.denoise(latents=lat, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                           sa_hidden_states=sa, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                           callback=callback, callback_steps=callback_steps or 1, trace=trace,
                           eta=eta, generator=generator, variance_noise=kwargs.get("variance_noise"),          # eta: :451, :530
                           requests=R, image_scale=scale_rows, guidance_rescale=guidance_rescale,
                           noise_plan=self._shard_noise(keyed, shard_over_ranks))
        return self._decode(out, output_type, generator)                                            # :544-547
