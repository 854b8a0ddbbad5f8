"""ControlNet-inpainting pipeline: per-step masked latent blend
(mirrors /root/reference/dressing_sd/pipelines/IMAGDressing_v1_pipeline_controlnet_inpainting.py:13-40, 117-548)."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ...unet import nchw_to_nhwc8
from ._base import (PipelineBase, RefSAttnProcessor2_0, RequestLayout, StableDiffusionPipelineOutput, as_batch,
                    min_guidance, multi_control_images, per_call_value, randn_tensor, set_scale_by_type, to_image_tensor, unipc_fused)


def _pil_images(value, name: str, mode: Optional[str]) -> list:
    """``image`` / ``mask_image`` of a call with ``padding_mask_crop``, ``overlay`` or the built-in inpaint condition: one PIL image or
    uint8 array ([H, W], [H, W, C]; [B, H, W, C]: one entry per row) or a list of them -> PIL images (converted to ``mode`` if given)"""
    import numpy as np
    from PIL import Image
    if value is None:
        raise ValueError(f"padding_mask_crop, overlay and control_image=None need {name} as a PIL image or uint8 array, got None")
    items = list(value) if isinstance(value, (list, tuple)) else [value]
    out = []
    for it in items:
        if hasattr(it, "convert") and hasattr(it, "resize"):
            out.append(it)
            continue
        a = None if isinstance(it, torch.Tensor) else np.asarray(it)
        if a is None or a.dtype != np.uint8 or a.ndim not in (2, 3, 4):
            raise ValueError(f"padding_mask_crop, overlay and control_image=None need {name} as a PIL image or uint8 array "
                             f"(latents and float tensors cannot be cropped or composited), got {type(it).__name__}")
        for row in (a if a.ndim == 4 else [a]):
            out.append(Image.fromarray(row[..., 0] if row.ndim == 3 and row.shape[-1] == 1 else row))
    if not out:
        raise ValueError(f"{name} is empty")
    return [im if mode is None or im.mode == mode else im.convert(mode) for im in out]


def _mask_filter_requests(mask_dilate, mask_blur, R: int):
    """``mask_dilate`` / ``mask_blur`` of a call, checked -> [(k, b)] * R, or None when every value is 0 (the call is then the one
    without the arguments).  A list gives one value per request: any other length raises ValueError."""
    from ...image import mask_filter_values

    def per_request(name, v):
        if isinstance(v, (list, tuple)):
            if len(v) != R:
                raise ValueError(f"{name} has {len(v)} entries for {R} requests (give one value, or one per request)")
            return list(v)
        return [v] * R
    vals = [mask_filter_values(k, b) for k, b in zip(per_request("mask_dilate", mask_dilate), per_request("mask_blur", mask_blur))]
    return vals if any(k > 0 or b > 0.0 for k, b in vals) else None


def _soft_mask_requests(soft_mask, R: int) -> Optional[List[bool]]:
    """``soft_mask`` of a call, checked -> R bools, or None when every value is False (the call is then the one without the argument).
    A list gives one value per request: any other length raises ValueError.  bool, ``numpy.bool_`` and the ints 0 / 1 are taken."""
    import numpy as np
    vals = list(soft_mask) if isinstance(soft_mask, (list, tuple)) else [soft_mask] * R
    if len(vals) != R:
        raise ValueError(f"soft_mask has {len(vals)} entries for {R} requests (give one value, or one per request)")
    for v in vals:
        if not isinstance(v, (bool, int, np.bool_)) or v not in (0, 1):
            raise ValueError(f"soft_mask takes True or False, got {v!r}")
    return [bool(v) for v in vals] if any(vals) else None


class _InpaintImages:
    """The person image(s) and mask(s) of a call that crops (``padding_mask_crop``), composites (``overlay``) or builds the inpaint
    condition itself: pair j = (image j, mask j) of request j (one pair: shared), its crop box, and its inputs on either image route --
    the host route through Pillow, the device route (``enable_device_image_io``) from ONE upload of each image as uint8, windows being
    tensor views."""

    def __init__(self, pipe, image, mask_image, size, pad, device, mask_filter=None):
        from ...image import crop_region_of_bounds, get_crop_region
        self.pipe, self.size, self.device = pipe, size, torch.device(device)          # size = (height, width), VAE multiples
        self.on_device = bool(getattr(pipe, "_device_image_io", False)) and self.device.type == "cuda"
        self._up = {}
        self.images, self.masks = _pil_images(image, "image", "RGB"), _pil_images(mask_image, "mask_image", None)
        self.n = max(len(self.images), len(self.masks))
        if len(self.images) not in (1, self.n) or len(self.masks) not in (1, self.n):
            raise ValueError(f"image has {len(self.images)} entries and mask_image {len(self.masks)} (give one, shared, or one per request)")
        self.masks_l = [m if m.mode == "L" else m.convert("L") for m in self.masks]
        for j in range(self.n):
            if self.image(j).size != self.mask(j).size:
                raise ValueError(f"image is {self.image(j).size} and mask_image {self.mask(j).size} (width, height): padding_mask_crop / "
                                 "overlay / control_image=None need them of equal size")
        self.cropped = pad is not None
        # mask_dilate / mask_blur on the device route (the host route hands in masks that are filtered already): mask j as "L" is
        # uploaded once, filtered by imd_image_mask_filter and stands where uploaded("mask_l", j) would; the crop box comes from the
        # bounds the last launch wrote, ONE copy of 16 bytes per mask for the call.  No reader sees the unfiltered mask.
        self.filtered = mask_filter is not None
        bounds = None
        if self.filtered:
            if not self.on_device or len(mask_filter) != len(self.masks):
                raise ValueError("mask_filter: one (dilate, blur) per mask, on the device image route")
            proc, ups, bnd = pipe._image_processor(), {}, []
            for j, (k, b) in enumerate(mask_filter):
                if id(self.masks[j]) not in ups:
                    ups[id(self.masks[j])] = proc._upload(self.masks_l[j], "L")
                res = proc.mask_filter(ups[id(self.masks[j])], k, b, bounds=self.cropped)
                self._up[("mask_l", j)] = res[0] if self.cropped else res
                if self.cropped:
                    bnd.append(res[1])
            self.masks_l = [None] * len(self.masks)               # (nothing may read the unfiltered "L" masks from here on)
            if self.cropped:
                bounds = torch.cat(bnd).cpu().tolist()
        if bounds is not None:
            self.boxes = [crop_region_of_bounds(bounds[j if len(self.masks) > 1 else 0], *self.image(j).size, size[1], size[0], pad=pad)
                          for j in range(self.n)]
        else:
            self.boxes = [get_crop_region(self.mask_l(j), size[1], size[0], pad=pad) if self.cropped
                          else (0, 0) + self.image(j).size for j in range(self.n)]

    def image(self, j):
        return self.images[j if len(self.images) > 1 else 0]

    def mask(self, j):
        return self.masks[j if len(self.masks) > 1 else 0]

    def mask_l(self, j):
        return self.masks_l[j if len(self.masks) > 1 else 0]

    def uploaded(self, kind: str, j: int) -> torch.Tensor:
        """uint8 [1, H0, W0, 3 | 1] on the device: kind "image" (RGB), "mask_l" (L) or "mask_rgb", uploaded once"""
        src, mode = {"image": (self.images, "RGB"), "mask_l": (self.masks_l, "L"), "mask_rgb": (self.masks, "RGB")}[kind]
        key = (kind, j if len(src) > 1 else 0)
        if key not in self._up:
            self._up[key] = self.pipe._image_processor()._upload(src[key[1]], mode)
        return self._up[key]

    @staticmethod
    def window(t: torch.Tensor, box) -> torch.Tensor:
        x1, y1, x2, y2 = box
        return t[:, y1:y2, x1:x2, :]

    def image_tensor(self, multiple: int) -> torch.Tensor:
        """the windows of the person images, Lanczos to the processing size, in [-1, 1]: fp32 [n, 3, H, W]"""
        if self.on_device:
            views = [self.window(self.uploaded("image", j), self.boxes[j]) for j in range(self.n)]
            return self.pipe._image_processor().preprocess(views, size=self.size, resample="lanczos", out="nchw", normalize=True, multiple=multiple)
        return to_image_tensor([self.image(j).crop(self.boxes[j]) for j in range(self.n)], self.device, True, size=self.size, multiple=multiple)

    def mask_latents(self, h: int, w: int) -> torch.Tensor:
        """the windows of the masks, binarised at 0.5 and nearest-resized to the latent size: fp32 [n, 1, h, w]"""
        rows = []
        for j in range(self.n):
            if self.on_device:
                gray = self.filtered or self.mask(j).mode in ("1", "L")          # (their RGB conversion repeats the one channel)
                view = self.window(self.uploaded("mask_l" if gray else "mask_rgb", j), self.boxes[j])
                m = self.pipe._image_processor().preprocess(view, size=None, out="nchw", normalize=False, binarize=True,
                                                            mode="L" if gray else "RGB")[:, :1]
            else:
                m = to_image_tensor(self.mask(j).crop(self.boxes[j]), self.device, False)[:, :1]
            rows.append(torch.nn.functional.interpolate((m >= 0.5).float(), size=(h, w)))
        return torch.cat(rows)

    def control(self, control_image, multiple: int) -> torch.Tensor:
        """the ControlNet image per pair: ``control_image`` (PIL / uint8: window, Lanczos; a float tensor [*, 3, H0, W0] of the image's
        size: window, nearest -- the -1 markers of ``make_inpaint_condition`` survive), or for None that condition built here at the
        processing size.  fp32 NCHW [n, 3, H, W] on the host route, the engines' NHWC8 on the device route."""
        from ...image import inpaint_condition_host
        if control_image is None:
            if self.on_device:
                proc = self.pipe._image_processor()
                return torch.cat([proc.inpaint_condition(self.uploaded("image", j), self.uploaded("mask_l", j), self.size,
                                                         self.boxes[j] if self.cropped else None) for j in range(self.n)])
            conds = [inpaint_condition_host(self.image(j), self.mask_l(j), self.boxes[j] if self.cropped else None, self.size)
                     for j in range(self.n)]
            return torch.stack([torch.from_numpy(c) for c in conds]).permute(0, 3, 1, 2).to(self.device)
        if isinstance(control_image, torch.Tensor):
            entries = [control_image[None]] if control_image.dim() == 3 else [control_image[i:i + 1] for i in range(control_image.shape[0])]
        else:
            entries = [e[None] if isinstance(e, torch.Tensor) and e.dim() == 3 else e
                       for e in (control_image if isinstance(control_image, (list, tuple)) else [control_image])]
        if len(entries) not in (1, self.n):
            raise ValueError(f"control_image has {len(entries)} entries for {self.n} image / mask pairs")
        rows = []
        for j in range(self.n):
            e, (x1, y1, x2, y2) = entries[j if len(entries) > 1 else 0], self.boxes[j]
            W0, H0 = self.image(j).size
            if isinstance(e, torch.Tensor):
                if not e.is_floating_point() or e.dim() != 4 or tuple(e.shape[-2:]) != (H0, W0):
                    raise ValueError(f"padding_mask_crop: a tensor control_image is a float [*, 3, {H0}, {W0}] tensor of the image's size "
                                     f"(only then the crop window is defined), got {e.dtype} {tuple(e.shape)}")
                rows.append(to_image_tensor(e[..., y1:y2, x1:x2], self.device, False, size=self.size, multiple=multiple))
                continue
            pil = _pil_images(e, "control_image", "RGB")[0]
            if pil.size != (W0, H0):
                raise ValueError(f"padding_mask_crop: control_image is {pil.size} and image {(W0, H0)} (width, height)")
            if self.on_device:
                view = self.window(self.pipe._image_processor()._upload(pil, "RGB"), self.boxes[j])
                rows.append(self.pipe._image_processor().preprocess(view, size=self.size, resample="lanczos", out="nhwc8", normalize=False,
                                                                    multiple=multiple))
            else:
                rows.append(to_image_tensor(pil.crop(self.boxes[j]), self.device, False, size=self.size, multiple=multiple))
        if any(r.shape[-1] == 8 and r.dtype == self.pipe.unet.dtype for r in rows):          # device route: every row in the engines' layout
            rows = [r if r.shape[-1] == 8 and r.dtype == self.pipe.unet.dtype else nchw_to_nhwc8(r.to(self.device), self.pipe.unet.dtype) for r in rows]
        return torch.cat(rows)


class IMAGDressing_v1(PipelineBase):
    _optional_components: list = []

    def __init__(self, vae, reference_unet, unet, tokenizer, text_encoder, controlnet, image_encoder, ImgProj, scheduler,
                 safety_checker=None, feature_extractor=None, requires_safety_checker: bool = True):
        self._init_common(vae=vae, reference_unet=reference_unet, unet=unet, tokenizer=tokenizer, text_encoder=text_encoder,
                          image_encoder=image_encoder, ImgProj=ImgProj, scheduler=scheduler, safety_checker=safety_checker,
                          feature_extractor=feature_extractor, controlnet=controlnet)

    def set_scale(self, scale):
        set_scale_by_type(self.unet, RefSAttnProcessor2_0, scale=scale)

    @property
    def mask_processor(self):
        """diffusers' ``pipe.mask_processor``: ``.blur(mask, blur_factor=4)`` -- Pillow for a PIL mask, ``imd_image_mask_filter`` for an
        uploaded uint8 one (``imagdressing_amd.image.MaskProcessor``)"""
        from ...image import MaskProcessor
        return MaskProcessor(self._image_processor)

    def _image_latents(self, image, device, generator, size=None):
        """VAE-encode the person image (inherited ``prepare_latents(..., return_image_latents=True)``, :330-346)."""
        p = next(self.vae.parameters())
        x = self._image_tensor(image, p.device, normalize=True, size=size, multiple=self.vae_scale_factor)[0].to(p.dtype)
        return self.vae.encode(x).latent_dist.sample(generator) * self.vae.config.scaling_factor

    def _decode_overlay(self, latents, output_type, front: _InpaintImages):
        """``_decode`` to uint8, then every image composited into its request's person image (``overlay=True``): the decoded image
        Lanczos-resized to the request's box, pasted, and ``Image.composite`` with the original through the unbinarised mask.  Host
        route: those Pillow calls.  Device route: pack, one resample and one ``imd_image_overlay`` launch per request, one copy back."""
        import numpy as np
        from ...image import overlay_host
        B = latents.shape[0]
        per = B // front.n if front.n > 1 else B                        # rows of one image / mask pair (request-major)
        if front.on_device:
            if not hasattr(self.vae, "decode_nhwc"):
                raise TypeError("enable_device_image_io() needs the engine VAE (imagdressing_amd.vae.AutoencoderKL.decode_nhwc), got "
                                f"{type(self.vae).__module__}.{type(self.vae).__name__}")
            proc = self._image_processor()
            parts = [proc.pack(y) for y in self._decode_nhwc(latents)]
            packed = parts[0] if len(parts) == 1 else torch.cat(parts)
            same = len({front.image(j).size for j in range(front.n)}) == 1
            W0, H0 = front.image(0).size
            whole = torch.empty(B, H0, W0, 3, dtype=torch.uint8, device=packed.device) if same else None
            outs = [proc.overlay(packed[j * per:(j + 1) * per], front.uploaded("image", j), front.uploaded("mask_l", j), front.boxes[j],
                                 out=None if whole is None else whole[j * per:(j + 1) * per]) for j in range(B // per)]
            arrs = list(whole.cpu().numpy()) if same else [a for o in outs for a in o.cpu().numpy()]
        else:
            dec = self._decode(latents, "np").images
            arrs = [np.asarray(overlay_host(dec[b], front.image(b // per), front.mask_l(b // per), front.boxes[b // per])) for b in range(B)]
        if output_type == "np":
            return StableDiffusionPipelineOutput(images=np.stack(arrs), nsfw_content_detected=None)
        from PIL import Image
        return StableDiffusionPipelineOutput(images=[Image.fromarray(a) for a in arrs], nsfw_content_detected=None)

    def _mask_release(self, mask_image, front: Optional[_InpaintImages], ups, h: int, w: int, n: int) -> torch.Tensor:
        """``soft_mask``: the release steps of every mask of the call, uint16 [masks, h, w] -- each mask read as "L" (filtered already
        where ``mask_dilate`` / ``mask_blur`` were given), its crop box's window under ``padding_mask_crop`` and whole otherwise.  Host
        route: ``mask_release_reference`` in numpy.  Device route: one ``imd_image_mask_release`` launch per mask on the uploaded bytes
        (``ups``: the plain route's filtered uploads), the window a view."""
        import numpy as np
        from ...image import mask_as_l, mask_release_reference
        if front is not None:                                 # (parsed, converted and -- device route -- uploaded there already)
            on_device = front.on_device
            count, boxes = len(front.masks), [front.boxes[j] if front.cropped else None for j in range(front.n)]
        else:                                                 # the plain route: the hard mask goes through _image_tensor, which keeps no images
            on_device = bool(getattr(self, "_device_image_io", False)) and torch.device(self.device).type == "cuda"
            try:
                masks = _pil_images(mask_image, "mask_image", None)
            except ValueError as e:
                raise ValueError(f"soft_mask reads mask_image as an 8-bit 'L' image: {e}") from None
            count, boxes = len(masks), [None] * len(masks)
        rows = []
        for j in range(count):
            if on_device:
                proc = self._image_processor()
                up = front.uploaded("mask_l", j) if front is not None else (ups[j] if ups is not None else proc._upload(masks[j], "L"))
                rows.append(proc.mask_release(up, h, w, n, boxes[j]).view(torch.int16))
            else:
                a = mask_as_l(front.mask_l(j) if front is not None else masks[j])
                if boxes[j] is not None:
                    x1, y1, x2, y2 = boxes[j]
                    a = a[y1:y2, x1:x2]
                rows.append(torch.from_numpy(mask_release_reference(np.ascontiguousarray(a), h, w, n)).view(torch.int16))
        return torch.stack(rows).view(torch.uint16)

    def open_session(self, *args, **kwargs):
        raise NotImplementedError("open_session on the inpainting pipeline: the per-row blend coefficients are in imd_sampler_step_rows, the per-slot mask / image-latent buffers are not built yet")

    @torch.no_grad()
    def __call__(self, prompt, null_prompt, negative_prompt, ref_image, width, height, num_inference_steps, guidance_scale,
                 ref_clip_image=None, num_images_per_prompt=1, image_scale=1.0, num_samples=1, strength: float = 1.0,
                 image=None, mask_image=None, control_image=None, padding_mask_crop: Optional[int] = None,
                 latents: Optional[torch.Tensor] = None, timesteps: List[int] = None,
                 callback_on_step_end: Optional[Callable] = None, callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 eta: float = 0.0, generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 output_type: Optional[str] = "pil", return_dict: bool = True, clip_skip: Optional[int] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 ref_clip_hidden_states: Optional[torch.Tensor] = None, ref_image_latents: Optional[torch.Tensor] = None,
                 image_latents: Optional[torch.Tensor] = None, mask_latents: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None, shard_over_ranks: bool = False, trace: Optional[list] = None,
                 mask_dilate: Union[int, List[int]] = 0, mask_blur: Union[float, List[float]] = 0.0,
                 soft_mask: Union[bool, List[bool]] = False, guidance_rescale: Union[float, List[float]] = 0.0,
                 overlay: bool = False, **kwargs):
        """``soft_mask`` (one bool, or a list with one per request; default False): the gray level of a mask pixel decides for how
        many of the LAST steps it is free to be repainted (Differential Diffusion, Levin & Fried 2023) instead of the mask being
        binarised at 0.5: the mask is read as "L" -- after ``mask_dilate`` / ``mask_blur``, inside the crop box of
        ``padding_mask_crop`` -- and ``image.mask_release_reference`` (host route) or ``imd_image_mask_release`` (device route) turns it
        into the release step of every latent pixel for the n = ``init_steps`` positions the call runs; ``mask_latents`` as a float
        tensor in [0, 1] is taken as the levels themselves (the tensor is read, never written).  ``mask_image`` must be a PIL image
        or a uint8 array (or a list of them) here, also on the plain route, where the hard mask takes a tensor too: gray levels are
        read from 8-bit "L" pixels, and a tensor ``mask_image`` raises ValueError -- pass it as ``mask_latents``.  Every step still blends with a 0 / 1 mask, written by ONE
        ``imd_soft_mask_rows`` launch in front of it; a request at False keeps its hard mask and its bits.

        ``mask_dilate`` = k and ``mask_blur`` = b (one value, or a list with one per request; 0: the step is skipped) grow and feather
        the mask before ANY reader sees it -- the crop box, the binarised latent mask, the built-in inpaint condition, the overlay and
        the plain route with a caller's ``control_image``: the call equals, byte for byte, the same call given each mask as
        ``m.convert("L").filter(ImageFilter.MaxFilter(2 k + 1)).filter(ImageFilter.GaussianBlur(b))`` (always "L" first, also for an
        RGB mask).  Host route: those Pillow calls.  ``enable_device_image_io()``: ``imd_image_mask_filter`` on the uploaded mask."""
        # several nets: control_image holds one entry per net (at most one None: the condition built here), checked below
        K = self._multi_control("control_image", control_image if control_image is not None else (), shard_over_ranks)
        R = self._request_count(dict(prompt=prompt, prompt_embeds=prompt_embeds, negative_prompt=negative_prompt, null_prompt=null_prompt,
                                     negative_prompt_embeds=negative_prompt_embeds, ref_image=ref_image, ref_clip_image=ref_clip_image,
                                     ref_clip_hidden_states=ref_clip_hidden_states, ref_image_latents=ref_image_latents,
                                     control_image=None if K else control_image, image=image, mask_image=mask_image, image_latents=image_latents,
                                     mask_latents=mask_latents, guidance_scale=guidance_scale, image_scale=image_scale,
                                     guidance_rescale=guidance_rescale),
                                dict(dict(num_inference_steps=num_inference_steps, strength=strength, eta=eta),
                                     **({} if K else dict(controlnet_conditioning_scale=controlnet_conditioning_scale))), shard_over_ranks,
                                control=None if K else dict(controlnet_conditioning_scale=controlnet_conditioning_scale,
                                                            control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end))
        control_images = multi_control_images("control_image", control_image, K, R, allow_none=1) if K else [control_image]
        builtin_condition = any(e is None for e in control_images)
        num_inference_steps, strength, eta = (per_call_value("num_inference_steps", num_inference_steps), per_call_value("strength", strength),
                                              per_call_value("eta", eta))
        if guess_mode or min_guidance(guidance_scale) <= 1.0 or timesteps:
            raise NotImplementedError("guess_mode, guidance_scale <= 1 and custom timesteps are not implemented "
                                      "(the reference script uses none of them)")
        soft_rows = _soft_mask_requests(soft_mask, R)
        if soft_rows is not None:
            if shard_over_ranks:
                raise NotImplementedError("soft_mask with shard_over_ranks: the release steps are built for the rows of one rank")
            if mask_image is None and mask_latents is None:
                raise ValueError("soft_mask reads the gray levels of mask_image (or of a float mask_latents); neither was given")
            if mask_latents is not None:
                if not isinstance(mask_latents, torch.Tensor) or not mask_latents.is_floating_point() or mask_latents.dim() != 4:
                    raise ValueError("soft_mask with mask_latents: a float [1 | R | B, 1, h, w] tensor of levels in [0, 1]")
                if not bool(torch.isfinite(mask_latents).all()) or float(mask_latents.min()) < 0.0 or float(mask_latents.max()) > 1.0:
                    raise ValueError("soft_mask: mask_latents must be finite and in [0, 1]")
        # mask_dilate / mask_blur: the host route swaps the filtered "L" masks in for mask_image here, before anything reads it; the
        # device route filters the uploaded masks (in _InpaintImages, or below for the plain route)
        mask_filter = _mask_filter_requests(mask_dilate, mask_blur, R)
        if mask_filter is not None:
            if mask_image is None:
                raise ValueError("mask_dilate / mask_blur filter mask_image; mask_latents cannot be dilated or blurred, and no mask_image was given")
            masks = _pil_images(mask_image, "mask_image", None)
            if len(masks) not in (1, R):
                raise ValueError(f"mask_image has {len(masks)} entries for {R} requests (give one, shared, or one per request)")
            if len(masks) == 1 and len(set(mask_filter)) > 1:
                masks = masks * R                                             # one mask, filtered differently per request
            mask_filter = mask_filter[:len(masks)]
            if getattr(self, "_device_image_io", False) and torch.device(self.device).type == "cuda":
                mask_image = masks if len(masks) > 1 else masks[0]
            else:
                from ...image import mask_filter_host
                done = [mask_filter_host(m, k, b) for m, (k, b) in zip(masks, mask_filter)]
                mask_image, mask_filter = (done if len(done) > 1 else done[0]), None
        # padding_mask_crop / overlay / control_image=None (the condition built here): the image and mask as images, one box per request
        front = None
        if padding_mask_crop is not None or overlay or (builtin_condition and image is not None and mask_image is not None):
            if padding_mask_crop is not None and (image_latents is not None or mask_latents is not None):
                raise ValueError("padding_mask_crop crops image and mask_image; image_latents / mask_latents cannot be cropped")
            if overlay and output_type not in ("pil", "np"):
                raise ValueError(f"overlay=True composites uint8 images: output_type must be 'pil' or 'np', got {output_type!r}")
            if overlay and shard_over_ranks:
                raise NotImplementedError("overlay=True with shard_over_ranks: each rank holds a part of the rows; composite per rank instead")
            vsf = self.vae_scale_factor
            front = _InpaintImages(self, image, mask_image, (height // vsf * vsf, width // vsf * vsf), padding_mask_crop, self.device,
                                   mask_filter=mask_filter)
            if overlay and output_type == "np" and len({front.image(j).size for j in range(front.n)}) > 1:
                raise ValueError("overlay=True with output_type='np' needs person images of one size (one array holds them); use 'pil'")
        if not 0.0 < float(strength) <= 1.0:
            raise ValueError(f"The value of strength should in (0.0, 1.0] but is {strength}")           # diffusers check_inputs (0.0 leaves no step)
        callback = kwargs.pop("callback", None)
        callback_steps = kwargs.pop("callback_steps", None) or 1
        scale, scale_rows = self._image_scales(image_scale, R)
        self.set_scale(scale)
        device = self.device
        self._cross_attention_kwargs = cross_attention_kwargs
        prompt_embeds, negative_prompt_embeds = self._request_prompts(
            R, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, device, clip_skip)
        ref_lat, cloth_tokens, G = self._request_garments(R, null_prompt, ref_image, ref_image_latents, ref_clip_image,
                                                          ref_clip_hidden_states, device)
        steps_run = min(int(num_inference_steps * float(strength)), num_inference_steps)          # the gate is over the timesteps actually run (:376-381)
        control_tensors = []
        for entry in control_images:
            if front is not None and (front.cropped or entry is None):
                control_tensors.append(front.control(entry, self.vae_scale_factor))
            else:
                control_tensors.append(self._image_tensor(as_batch(entry, "control_image"), device, normalize=False, size=(height, width),
                                                          multiple=self.vae_scale_factor, layout="nhwc8")[0])
        if K:          # the mix route: ``multi_rows[k][r][i]``, the effective scale of net k for request r at every step that runs
            control = dict(image=control_tensors, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, scale=1.0,
                           multi_rows=self._multi_control_plan(controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                                                               K, R, max(steps_run, 1)))
        else:
            # (enable_request_control_scales and differing triples: ``rows``, the effective scale of every request at every step that runs)
            ctrl_scale, ctrl_keep, ctrl_rows = self._control_plan(controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                                                                  R, max(steps_run, 1))
            control = dict(image=control_tensors[0],
                           prompt_embeds=prompt_embeds,
                           negative_prompt_embeds=negative_prompt_embeds, scale=ctrl_scale, keep=ctrl_keep, rows=ctrl_rows)
        B = R * num_images_per_prompt
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        # strength == 1.0: start from pure noise; the SAME noise re-noises the original latents in the blend (:496-498).
        # strength < 1.0 (:316-341 -> diffusers get_timesteps / prepare_latents): run the last int(steps * strength) timesteps,
        # starting from add_noise(image_latents, noise, first of them).  Explicit ``latents`` are taken as the noise, as diffusers does.
        if image_latents is None and front is not None and front.cropped:
            p = next(self.vae.parameters())
            x = front.image_tensor(self.vae_scale_factor).to(device=p.device, dtype=p.dtype)
            image_latents = self.vae.encode(x).latent_dist.sample(generator) * self.vae.config.scaling_factor
        elif image_latents is None:                                           # (before the noise draw, like diffusers' prepare_latents)
            image_latents = self._image_latents(as_batch(image, "image"), device, generator, size=(height, width))
        keyed = self._request_noise(kwargs, generator, R, num_images_per_prompt)          # enable_device_noise: one key per latent row
        if noise is None and latents is None and keyed is not None:
            noise = keyed.initial(h, w)          # draw 0: the initial noise, add_noise's noise and the blend's, as below
        if noise is None:
            noise = latents if latents is not None else randn_tensor((B, 4, h, w), generator=generator, device=device, dtype=torch.float32)
        init_steps = min(int(num_inference_steps * float(strength)), num_inference_steps)
        t_start = max(num_inference_steps - init_steps, 0)
        if init_steps < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline "
                             f"steps is {init_steps} which is < 1 and not appropriate for this pipeline.")
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        if latents is not None or float(strength) == 1.0:
            lat = (noise if latents is None else latents).to(device=device, dtype=torch.float32) * self.scheduler.init_noise_sigma
        else:
            # (unrounded: Euler's may be fractional; the fused UniPC step makes one UNet call per entry whatever its solver order)
            t0 = self.scheduler.timesteps[t_start * (1 if unipc_fused(self.scheduler) else getattr(self.scheduler, "order", 1))]
            il = image_latents.to(device=device, dtype=torch.float32)
            if il.shape[0] != B:                                              # one person image shared, or one per request (request-major rows)
                il = il.expand(B, -1, -1, -1) if il.shape[0] == 1 else RequestLayout(R, num_images_per_prompt).expand(il, "image / image_latents")
            lat = self.scheduler.add_noise(il, noise.to(device=device, dtype=torch.float32), t0)
        ups = release = None
        if soft_rows is not None and mask_latents is not None:                # the caller's levels, [1 | R | B, 1, h, w] in [0, 1]
            from ...image import release_of_levels
            release = torch.from_numpy(release_of_levels(mask_latents[:, 0], init_steps))
        if mask_latents is None and front is not None and front.cropped:
            mask_latents = front.mask_latents(h, w)
        elif mask_latents is None and mask_filter is not None:                # (device route: the uploaded masks, filtered; then as below)
            proc = self._image_processor()
            if front is not None:                                             # (filtered there already)
                ups = [front.uploaded("mask_l", j) for j in range(len(front.masks))]
            else:
                masks = mask_image if isinstance(mask_image, list) else [mask_image]
                raw = {id(mk): proc._upload(mk, "L") for mk in {id(mk): mk for mk in masks}.values()}          # (a shared mask is uploaded once)
                ups = [proc.mask_filter(raw[id(mk)], k, b) for mk, (k, b) in zip(masks, mask_filter)]
            m = proc.preprocess(ups, size=None, resample="lanczos", out="nchw", normalize=False, binarize=True, multiple=8, mode="L")[:, :1]
            mask_latents = torch.nn.functional.interpolate((m >= 0.5).float(), size=(h, w))
        elif mask_latents is None:                                            # prepare_mask_latents: nearest resize to h x w
            m = self._image_tensor(as_batch(mask_image, "mask_image"), device, normalize=False, binarize=True)[0][:, :1]
            m = (m >= 0.5).float()
            mask_latents = torch.nn.functional.interpolate(m, size=(h, w))
        lat, noise_s = self._shard(lat, shard_over_ranks), self._shard(noise.to(device), shard_over_ranks)
        sa = self._sa_states(ref_lat, cloth_tokens, shard_over_ranks, G)
        inpaint = dict(mask=mask_latents, image_latents=image_latents, noise=noise_s)
        if soft_rows is not None:
            if release is None:
                release = self._mask_release(mask_image, front, ups, h, w, init_steps)
            inpaint.update(release=release, soft_rows=soft_rows)
        out = self.denoise(latents=lat, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                           sa_hidden_states=sa, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                           control=control, inpaint=inpaint, callback=callback, callback_steps=callback_steps, trace=trace,
                           eta=eta, generator=generator, variance_noise=kwargs.get("variance_noise"), t_start=t_start,
                           requests=R, image_scale=scale_rows, guidance_rescale=guidance_rescale,
                           noise_plan=self._shard_noise(keyed, shard_over_ranks))
        if overlay:
            return self._decode_overlay(out, output_type, front)
        return self._decode(out, output_type, generator)
