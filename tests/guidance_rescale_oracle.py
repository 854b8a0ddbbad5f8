"""float64 restatement of the CFG rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", section
3.4; diffusers' ``rescale_noise_cfg``) as ``imd_guidance_rescale`` applies it to eps [2B, HW, 4] -- rows [0, B) cond, [B, 2B) uncond --
and the reference denoising loop with the rescale between the guidance and the scheduler step.  Parity with diffusers itself stays
unpinned (as for FreeU and UniPC): :func:`rescale_noise_cfg_literal` is the library's function restated, used to check this oracle."""
import torch


def _per_row(v, B):
    t = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    return t.expand(B) if t.numel() == 1 else t


def factors(eps, guidance, rescale):
    """-> (e [B, HW, 4] float64 guided prediction, f [B] float64 factor; f = 1 where S_e == 0) from eps in any float type"""
    x = eps.detach().cpu().double()
    B = x.shape[0] // 2
    t, u = x[:B], x[B:]
    g, phi = _per_row(guidance, B), _per_row(rescale, B)
    e = u + g.view(B, 1, 1) * (t - u)
    s_t = ((t - t.mean(dim=(1, 2), keepdim=True)) ** 2).sum(dim=(1, 2))
    s_e = ((e - e.mean(dim=(1, 2), keepdim=True)) ** 2).sum(dim=(1, 2))
    r = torch.where(s_e == 0, torch.ones_like(s_e), torch.sqrt(s_t / torch.where(s_e == 0, torch.ones_like(s_e), s_e)))
    return e, phi * r + (1 - phi)


def guidance_rescale(eps, guidance, rescale):
    """eps [2B, HW, 4] -> float64 [2B, HW, 4]: rows b and B + b = f e where rescale_b != 0, the input where it is 0"""
    x = eps.detach().cpu().double()
    B = x.shape[0] // 2
    e, f = factors(eps, guidance, rescale)
    out = x.clone()
    on = _per_row(rescale, B) != 0
    fe = f.view(B, 1, 1) * e
    out[:B][on] = fe[on]
    out[B:][on] = fe[on]
    return out


def rescale_noise_cfg_literal(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers' rescale_noise_cfg, line for line, on [B, C, H, W]-like tensors (std over every non-batch dimension)"""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


@torch.no_grad()
def denoise_rescaled(unet, reference_unet, scheduler, latents, prompt_embeds, negative_prompt_embeds, cloth_embeds, ref_latents,
                     num_inference_steps, guidance_scale, guidance_rescale=0.0):
    """oracle.pipeline.denoise of the base pipeline (no ControlNet, no blend) with the rescale applied to the guided prediction in
    float64 in front of ``scheduler.step``; at guidance_rescale = 0 it is that loop"""
    from oracle.pipeline import garment_features
    sa = None
    for i, t in enumerate(scheduler.set_timesteps(num_inference_steps)):
        if i == 0:
            sa = garment_features(reference_unet, ref_latents, cloth_embeds)
        lmi = scheduler.scale_model_input(torch.cat([latents] * 2), t)
        eps_c = unet(lmi[0:1], t, prompt_embeds, cross_attention_kwargs={"sa_hidden_states": sa})
        eps_u = unet(lmi[1:2], t, negative_prompt_embeds)
        eps = eps_u + guidance_scale * (eps_c - eps_u)
        if guidance_rescale:
            eps = rescale_noise_cfg_literal(eps.double(), eps_c.double(), guidance_rescale).to(eps.dtype)
        latents = scheduler.step(eps, t, latents)
    return latents
