"""Pipeline with IP-Adapter-FaceID-Plus face tokens + pose ControlNet
(mirrors /root/reference/dressing_sd/pipelines/IMAGDressing_v1_pipeline_ipa_controlnet.py:22-101, 366-742)."""
from __future__ import annotations

import os
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ...adapter.resampler import ProjPlusModel
from ._base import (IPAttnProcessor2_0, LoRAIPAttnProcessor2_0, LoraRefSAttnProcessor2_0, PipelineBase, as_batch,
                    min_guidance, multi_control_images, per_call_value, request_rows, set_scale_by_type)


def _faces(name, value):
    """a per-request face argument: a list whose entries are all None is no face; a list mixing None and faces raises"""
    if isinstance(value, (list, tuple)):
        present = [v is not None for v in value]
        if any(present) and not all(present):
            raise ValueError(f"{name} mixes requests with and without a face: one IP-Adapter call is all with faces or all without")
        if not any(present):
            return None
    return as_batch(value, name)


class IMAGDressing_v1(PipelineBase):
    _optional_components: list = []

    def __init__(self, vae, reference_unet, unet, tokenizer, text_encoder, controlnet, image_encoder, ImgProj, ip_ckpt, scheduler,
                 safety_checker=None, feature_extractor=None):
        self._init_common(vae=vae, reference_unet=reference_unet, unet=unet, tokenizer=tokenizer, text_encoder=text_encoder,
                          image_encoder=image_encoder, ImgProj=ImgProj, scheduler=scheduler, safety_checker=safety_checker,
                          feature_extractor=feature_extractor, controlnet=controlnet)
        self.ip_ckpt = ip_ckpt
        self.num_tokens = 4
        self.image_proj_model = self.init_proj()
        if ip_ckpt is not None:
            self.load_ip_adapter()

    def init_proj(self):                                                     # :79-86
        clip_dim = 1280
        if self.image_encoder is not None and hasattr(self.image_encoder, "config"):
            clip_dim = self.image_encoder.config.hidden_size
        return ProjPlusModel(cross_attention_dim=self.unet.config.cross_attention_dim, id_embeddings_dim=512,
                             clip_embeddings_dim=clip_dim, num_tokens=self.num_tokens)

    def load_ip_adapter(self):                                               # :88-101
        if isinstance(self.ip_ckpt, dict):
            state_dict = self.ip_ckpt
        elif os.path.splitext(self.ip_ckpt)[-1] == ".safetensors":
            from safetensors import safe_open
            state_dict = {"image_proj": {}, "ip_adapter": {}}
            with safe_open(self.ip_ckpt, framework="pt", device="cpu") as f:
                for key in f.keys():
                    if key.startswith("image_proj."):
                        state_dict["image_proj"][key.replace("image_proj.", "")] = f.get_tensor(key)
                    elif key.startswith("ip_adapter."):
                        state_dict["ip_adapter"][key.replace("ip_adapter.", "")] = f.get_tensor(key)
        else:
            state_dict = torch.load(self.ip_ckpt, map_location="cpu")
        self.image_proj_model.load_state_dict(state_dict["image_proj"])
        ip_layers = torch.nn.ModuleList([p for p in self.unet.attn_processors.values()])
        ip_layers.load_state_dict(state_dict["ip_adapter"], strict=False)

    def get_image_embeds(self, clip_image=None, faceid_embeds=None, clip_hidden_states=None, uncond_clip_hidden_states=None):
        """(face tokens, uncond face tokens) [1, 4, 768] each (:366-377).  ``shortcut`` stays False (:375)."""
        dev = self.device
        if clip_hidden_states is None:
            clip_hidden_states = self._clip_hidden(clip_image, dev)
            uncond_clip_hidden_states = self._clip_hidden(torch.zeros_like(clip_image), dev)
        faceid_embeds = faceid_embeds.to(dev)
        pos = self.image_proj_model(faceid_embeds, clip_hidden_states.to(dev))
        neg = self.image_proj_model(torch.zeros_like(faceid_embeds), uncond_clip_hidden_states.to(dev))
        return pos, neg

    def set_scale(self, scale, lora_scale):                                  # :379-383
        set_scale_by_type(self.unet, LoraRefSAttnProcessor2_0, scale=scale, lora_scale=lora_scale)

    def set_ipa_scale(self, ipa_scale, lora_scale):                          # :386-393
        set_scale_by_type(self.unet, LoRAIPAttnProcessor2_0, scale=ipa_scale, lora_scale=lora_scale)
        set_scale_by_type(self.unet, IPAttnProcessor2_0, scale=ipa_scale, lora_scale=lora_scale)

    def open_session(self, *args, **kwargs):
        raise NotImplementedError("open_session on the IP-Adapter pipeline: per-slot face tokens and LoRA scales are not built yet")

    @torch.no_grad()
    def __call__(self, prompt, null_prompt, negative_prompt, ref_image, width, height, num_inference_steps, guidance_scale,
                 pose_image=None, ref_clip_image=None, face_clip_image=None, faceid_embeds=None, num_images_per_prompt=1,
                 image_scale=1.0, ipa_scale=0.0, s_lora_scale=0.0, c_lora_scale=0.0, num_samples=1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, clip_skip: Optional[int] = None, callback: Optional[Callable] = None,
                 callback_steps: Optional[int] = 1, prompt_embeds: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 ref_clip_hidden_states: Optional[torch.Tensor] = None, ref_image_latents: Optional[torch.Tensor] = None,
                 face_clip_hidden_states: Optional[torch.Tensor] = None, face_uncond_clip_hidden_states: Optional[torch.Tensor] = None,
                 latents: Optional[torch.Tensor] = None, shard_over_ranks: bool = False, trace: Optional[list] = None,
                 guidance_rescale: Union[float, List[float]] = 0.0, **kwargs):
        rows_on = bool(getattr(self, "_request_adapter_scales", False))          # enable_request_adapter_scales
        adapter = dict(ipa_scale=ipa_scale, s_lora_scale=s_lora_scale, c_lora_scale=c_lora_scale)
        K = self._multi_control("pose_image", pose_image, shard_over_ranks)          # >= 2: per-net lists, checked below
        R = self._request_count(dict(prompt=prompt, prompt_embeds=prompt_embeds, negative_prompt=negative_prompt, null_prompt=null_prompt,
                                     negative_prompt_embeds=negative_prompt_embeds, ref_image=ref_image, ref_clip_image=ref_clip_image,
                                     ref_clip_hidden_states=ref_clip_hidden_states, ref_image_latents=ref_image_latents,
                                     pose_image=None if K else pose_image, face_clip_image=face_clip_image, faceid_embeds=faceid_embeds,
                                     face_clip_hidden_states=face_clip_hidden_states,
                                     face_uncond_clip_hidden_states=face_uncond_clip_hidden_states,
                                     guidance_scale=guidance_scale, image_scale=image_scale, guidance_rescale=guidance_rescale),
                                dict(dict(num_inference_steps=num_inference_steps, eta=eta),
                                     **({} if K else dict(controlnet_conditioning_scale=controlnet_conditioning_scale)),
                                     **({} if rows_on else adapter)), shard_over_ranks,
                                control=None if K else dict(controlnet_conditioning_scale=controlnet_conditioning_scale,
                                                            control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end))
        num_inference_steps, eta = per_call_value("num_inference_steps", num_inference_steps), per_call_value("eta", eta)
        adapter_rows = None
        if rows_on:
            # each argument on its own: equal values keep the folded route (set_scale / set_ipa_scale below, bit for bit); differing ones ride
            # in rows, read by the processors INSTEAD of their own attribute, which gets the neutral value (no LoRA folded; face weight 1)
            ipa_scale, ip_rows = self._adapter_scales("ipa_scale", ipa_scale, R, 1.0)
            s_lora_scale, s_rows = self._adapter_scales("s_lora_scale", s_lora_scale, R, 0.0)
            c_lora_scale, c_rows = self._adapter_scales("c_lora_scale", c_lora_scale, R, 0.0)
            adapter_rows = dict(s_lora_rows=s_rows, c_lora_rows=c_rows, ip_scale_rows=ip_rows)
        elif R > 1:
            ipa_scale, s_lora_scale, c_lora_scale = (per_call_value("ipa_scale", ipa_scale), per_call_value("s_lora_scale", s_lora_scale),
                                                     per_call_value("c_lora_scale", c_lora_scale))
        if guess_mode or min_guidance(guidance_scale) <= 1.0:
            # neither runs in the reference: with guess_mode its ControlNet sees the cond half only and the loop then indexes
            # down_block[1] of a batch-1 tensor (..._ipa_controlnet.py:634-639, :662-665; the zero-padding lines are commented out);
            # without CFG latent_model_input[1] does not exist (:672, :690)
            raise NotImplementedError("guess_mode / guidance_scale <= 1: the reference's loop indexes the CFG pair of the ControlNet "
                                      "residuals and of the latents unconditionally (..._ipa_controlnet.py:662-690)")
        # the face tokens ride in the text context of every row: one call has a face for every request or for none
        face_clip_image, faceid_embeds = _faces("face_clip_image", face_clip_image), _faces("faceid_embeds", faceid_embeds)
        face_clip_hidden_states = _faces("face_clip_hidden_states", face_clip_hidden_states)
        face_uncond_clip_hidden_states = _faces("face_uncond_clip_hidden_states", face_uncond_clip_hidden_states)
        has_face = face_clip_image is not None or face_clip_hidden_states is not None
        scale, scale_rows = self._image_scales(image_scale, R)
        if not has_face:                                                      # :432-437
            self.set_scale(scale, lora_scale=0.0)
            self.set_ipa_scale(ipa_scale=0.0, lora_scale=0.0)
            adapter_rows = None                                               # (the three scales are not read without a face)
        else:
            self.set_scale(scale, lora_scale=s_lora_scale)
            self.set_ipa_scale(ipa_scale, lora_scale=c_lora_scale)
        device = self.device
        self._cross_attention_kwargs = cross_attention_kwargs
        prompt_embeds, negative_prompt_embeds = self._request_prompts(
            R, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, device, clip_skip)
        control = None
        if K:                                                                 # several nets: one pose_image entry per net, the mix route
            tensors = [self._image_tensor(as_batch(im, "pose_image"), device, normalize=False, size=(height, width),
                                          multiple=self.vae_scale_factor, layout="nhwc8")
                       for im in multi_control_images("pose_image", pose_image, K, R)]
            if len({hw for _, hw in tensors}) > 1:
                raise ValueError(f"pose_image: the images of the {K} ControlNets differ in size ({[hw for _, hw in tensors]}) after resizing")
            height, width = tensors[0][1]
            control = dict(image=[t for t, _ in tensors], prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, scale=1.0,
                           multi_rows=self._multi_control_plan(controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                                                               K, R, num_inference_steps))
        elif pose_image is not None:                                          # ControlNet sees the 77 text tokens only (:550)
            image, (height, width) = self._image_tensor(as_batch(pose_image, "pose_image"), device, normalize=False, size=(height, width),
                                                        multiple=self.vae_scale_factor, layout="nhwc8")
            # (enable_request_control_scales and differing triples: ``rows``, the effective scale of every request at every step)
            ctrl_scale, ctrl_keep, ctrl_rows = self._control_plan(controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                                                                  R, num_inference_steps)
            control = dict(image=image, prompt_embeds=prompt_embeds,
                           negative_prompt_embeds=negative_prompt_embeds, scale=ctrl_scale, keep=ctrl_keep, rows=ctrl_rows)
        if has_face:                                                          # :513-521, :555-557
            pos, neg = self.get_image_embeds(face_clip_image, faceid_embeds, face_clip_hidden_states, face_uncond_clip_hidden_states)
            if R > 1:                                                         # one face per request (or one shared by all)
                pos, neg = request_rows(pos, R, "face tokens"), request_rows(neg, R, "uncond face tokens")
            prompt_embeds = torch.cat([prompt_embeds.to(device), pos.to(prompt_embeds.dtype)], dim=1)
            negative_prompt_embeds = torch.cat([negative_prompt_embeds.to(device), neg.to(negative_prompt_embeds.dtype)], dim=1)
        ref_lat, cloth_tokens, G = self._request_garments(R, null_prompt, ref_image, ref_image_latents, ref_clip_image,
                                                          ref_clip_hidden_states, device)
        self.scheduler.set_timesteps(num_inference_steps, device=device)      # (init_noise_sigma may depend on the schedule; IMAGDressing_v1_pipeline.py:386)
        keyed = self._request_noise(kwargs, generator, R, num_images_per_prompt)          # enable_device_noise: one key per latent row
        lat = self._shard(self.prepare_latents(R * num_images_per_prompt, 4, width, height, torch.float32, device, generator, latents,
                                               noise_plan=keyed), shard_over_ranks)
        sa = self._sa_states(ref_lat, cloth_tokens, shard_over_ranks, G)
        out = self.denoise(latents=lat, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                           sa_hidden_states=sa, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                           control=control, callback=callback, callback_steps=callback_steps or 1, trace=trace,
                           eta=eta, generator=generator, variance_noise=kwargs.get("variance_noise"), requests=R, image_scale=scale_rows,
                           adapter_rows=adapter_rows, guidance_rescale=guidance_rescale,
                           noise_plan=self._shard_noise(keyed, shard_over_ranks))
        return self._decode(out, output_type, generator)
