"""Pipeline with an optional pose ControlNet
(mirrors /root/reference/dressing_sd/pipelines/IMAGDressing_v1_pipeline_controlnet.py:20-45, 352-677)."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ._base import PipelineBase, RefSAttnProcessor2_0, as_batch, min_guidance, multi_control_images, per_call_value, set_scale_by_type


class IMAGDressing_v1(PipelineBase):
    _optional_components: list = []

    def __init__(self, vae, reference_unet, unet, tokenizer, text_encoder, controlnet, image_encoder, ImgProj, scheduler,
                 safety_checker=None, feature_extractor=None):
        self._init_common(vae=vae, reference_unet=reference_unet, unet=unet, tokenizer=tokenizer, text_encoder=text_encoder,
                          image_encoder=image_encoder, ImgProj=ImgProj, scheduler=scheduler, safety_checker=safety_checker,
                          feature_extractor=feature_extractor, controlnet=controlnet)

    def set_scale(self, scale):                                              # :352-355
        set_scale_by_type(self.unet, RefSAttnProcessor2_0, scale=scale)

    def _control(self, pose_image, prompt_embeds, negative_prompt_embeds, num_inference_steps, scale, start, end, device, size=None, requests=1):
        """ControlNet inputs: the pose image (shared by the CFG halves, :497-498) and the TEXT-ONLY embeddings
        (``prompt_embeds_control``, ..._ipa_controlnet.py:550).  ``rows``: None (the folded route), or with
        ``enable_request_control_scales`` and differing (scale, start, end) the effective scale of every request at every step."""
        if pose_image is None:
            return None
        image, hw = self._image_tensor(pose_image, device, normalize=False, size=size, multiple=self.vae_scale_factor, layout="nhwc8")
        scale, keep, rows = self._control_plan(scale, start, end, requests, num_inference_steps)
        return dict(image=image, hw=hw, prompt_embeds=prompt_embeds,
                    negative_prompt_embeds=negative_prompt_embeds, scale=scale, keep=keep, rows=rows)

    def _controls(self, K, pose_image, prompt_embeds, negative_prompt_embeds, num_inference_steps, scale, start, end, device, size=None, requests=1):
        """``_control`` for K >= 2 nets: ``pose_image`` holds one entry per net; ``multi_rows[k][r][i]`` is the effective scale of net k
        for request r at step i (the mix route, whatever the values)."""
        tensors = [self._image_tensor(as_batch(im, "pose_image"), device, normalize=False, size=size, multiple=self.vae_scale_factor,
                                      layout="nhwc8") for im in multi_control_images("pose_image", pose_image, K, requests)]
        if len({hw for _, hw in tensors}) > 1:
            raise ValueError(f"pose_image: the images of the {K} ControlNets differ in size ({[hw for _, hw in tensors]}) after resizing")
        rows = self._multi_control_plan(scale, start, end, K, requests, num_inference_steps)
        return dict(image=[t for t, _ in tensors], hw=tensors[0][1], prompt_embeds=prompt_embeds,
                    negative_prompt_embeds=negative_prompt_embeds, scale=1.0, multi_rows=rows)

    def open_session(self, slots: int, width: int, height: int, controlnet_conditioning_scale: float = 1.0, compact: bool = False, widths=None,
                     device_noise: Optional[bool] = None, control_rows: Optional[bool] = None):
        """In-flight batching: a :class:`imagdressing_amd.session.DenoiseSession` with ``slots`` slots at ``width`` x ``height``; every
        request brings its own pose image, ``controlnet_conditioning_scale`` holds for the whole session (the gate is one scalar per
        launch) unless ``control_rows`` (None = follow ``enable_request_control_scales``): then ``submit`` takes
        ``controlnet_conditioning_scale`` (None: the value given here), ``control_guidance_start`` and ``control_guidance_end`` per
        request and every step runs one ``imd_residual_scale_rows`` launch behind the ControlNet, whatever the values.  A pipeline
        built without a ControlNet opens the session of the base pipeline.  ``compact`` / ``widths``: run only as many batch rows as
        requests are running; ``device_noise``: per-request seeded noise, None = follow ``enable_device_noise`` (``_open_session``)."""
        return self._open_session(slots, width, height, controlnet_conditioning_scale, with_controlnet=self.controlnet is not None,
                                  compact=compact, widths=widths, device_noise=device_noise, control_rows=control_rows)

    @torch.no_grad()
    def __call__(self, prompt, null_prompt, negative_prompt, ref_image, width, height, num_inference_steps, guidance_scale,
                 pose_image=None, ref_clip_image=None, num_images_per_prompt=1, image_scale=1.0, num_samples=1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, clip_skip: Optional[int] = None, callback: Optional[Callable] = None,
                 callback_steps: Optional[int] = 1, prompt_embeds: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 ref_clip_hidden_states: Optional[torch.Tensor] = None, ref_image_latents: Optional[torch.Tensor] = None,
                 latents: Optional[torch.Tensor] = None, shard_over_ranks: bool = False, trace: Optional[list] = None,
                 guidance_rescale: Union[float, List[float]] = 0.0, **kwargs):
        K = self._multi_control("pose_image", pose_image, shard_over_ranks)          # >= 2: per-net lists, checked in _controls
        R = self._request_count(dict(prompt=prompt, prompt_embeds=prompt_embeds, negative_prompt=negative_prompt, null_prompt=null_prompt,
                                     negative_prompt_embeds=negative_prompt_embeds, ref_image=ref_image, ref_clip_image=ref_clip_image,
                                     ref_clip_hidden_states=ref_clip_hidden_states, ref_image_latents=ref_image_latents,
                                     pose_image=None if K else pose_image, guidance_scale=guidance_scale, image_scale=image_scale,
                                     guidance_rescale=guidance_rescale),
                                dict(dict(num_inference_steps=num_inference_steps, eta=eta),
                                     **({} if K else dict(controlnet_conditioning_scale=controlnet_conditioning_scale))),
                                shard_over_ranks,
                                control=None if K else dict(controlnet_conditioning_scale=controlnet_conditioning_scale,
                                                            control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end))
        num_inference_steps, eta = per_call_value("num_inference_steps", num_inference_steps), per_call_value("eta", eta)
        if guess_mode or min_guidance(guidance_scale) <= 1.0:
            # neither runs in the reference: with guess_mode its ControlNet sees the cond half only and the loop then indexes
            # down_block[1] of a batch-1 tensor (..._ipa_controlnet.py:634-639, :662-665; the zero-padding lines are commented out);
            # without CFG latent_model_input[1] does not exist (:672, :690)
            raise NotImplementedError("guess_mode / guidance_scale <= 1: the reference's loop indexes the CFG pair of the ControlNet "
                                      "residuals and of the latents unconditionally (..._ipa_controlnet.py:662-690)")
        scale, scale_rows = self._image_scales(image_scale, R)
        self.set_scale(scale)
        device = self.device
        self._cross_attention_kwargs = cross_attention_kwargs
        prompt_embeds, negative_prompt_embeds = self._request_prompts(
            R, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, device, clip_skip)
        ref_lat, cloth_tokens, G = self._request_garments(R, null_prompt, ref_image, ref_image_latents, ref_clip_image,
                                                          ref_clip_hidden_states, device)
        if K:
            control = self._controls(K, pose_image, prompt_embeds, negative_prompt_embeds, num_inference_steps,
                                     controlnet_conditioning_scale, control_guidance_start, control_guidance_end, device,
                                     size=(height, width), requests=R)
        else:
            control = self._control(as_batch(pose_image, "pose_image"), prompt_embeds, negative_prompt_embeds, num_inference_steps,
                                    controlnet_conditioning_scale, control_guidance_start, control_guidance_end, device,
                                    size=(height, width), requests=R)
        if control is not None:
            height, width = control["hw"]                                   # :501
        self.scheduler.set_timesteps(num_inference_steps, device=device)      # (init_noise_sigma may depend on the schedule; IMAGDressing_v1_pipeline.py:386)
        keyed = self._request_noise(kwargs, generator, R, num_images_per_prompt)          # enable_device_noise: one key per latent row
        lat = self._shard(self.prepare_latents(R * num_images_per_prompt, 4, width, height, torch.float32, device, generator, latents,
                                               noise_plan=keyed), shard_over_ranks)
        sa = self._sa_states(ref_lat, cloth_tokens, shard_over_ranks, G)
        out = self.denoise(latents=lat, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                           sa_hidden_states=sa, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                           control=control, callback=callback, callback_steps=callback_steps or 1, trace=trace,
                           eta=eta, generator=generator, variance_noise=kwargs.get("variance_noise"), requests=R, image_scale=scale_rows,
                           guidance_rescale=guidance_rescale, noise_plan=self._shard_noise(keyed, shard_over_ranks))
        return self._decode(out, output_type, generator)
