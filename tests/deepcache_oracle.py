"""DeepCache on the CPU oracle (TEST INFRASTRUCTURE; helper, not collected): ``oracle.sd15.UNet2DConditionModel`` /
``ControlNetModel`` wrapped in callables of the same signature that apply the full / shallow rule through the oracle's own
sub-modules, following ``deepcache_plan`` -- so ``oracle.pipeline.denoise`` drives them unchanged.

The rule (L = layers_per_block, depth d in 1 .. L + 1): the down path pushes skips s0 = conv_in's output and s1 .. sL = the outputs of
the L layers of ``down_blocks[0]``; the last up block has L + 1 layers and layer j consumes s(L - j); F_d is the hidden state that
enters layer L + 1 - d of that block, before the concatenation with its skip.  A full call is the plain forward and keeps F_d; a
shallow call runs conv_in, layers 0 .. d - 2 of ``down_blocks[0]``, takes F_d from the last full call of ITS stream and runs layers
L + 1 - d .. L of the last up block and the output convolution.  The oracle loop calls the UNet twice per step at batch 1 (cond, then
uncond): ``streams`` = 2 gives each its own F_d and call count; the ControlNet is called once per step (``streams`` = 1).
"""
import torch
import torch.nn.functional as F

from imagdressing_amd.dressing_sd.pipelines._base import deepcache_plan


def _layer(block, j, x, temb, ehs, cak):
    x = block.resnets[j](x, temb)
    if block.has_attn:
        x = block.attentions[j](x, ehs, cak)
    return x


def unet_forward(m, sample, timestep, ehs, cak=None, ctrl=None, mid_res=None, depth=1, feat=None):
    """-> (eps, F_depth).  ``feat`` None: the full forward (== ``m(sample, timestep, ehs, ...)``), F_d captured on the way;
    otherwise the shallow forward around ``feat`` (``ctrl``: the first ``depth`` ControlNet residuals are read)."""
    cak = dict(cak or {})
    L = len(m.down_blocks[0].resnets)
    assert 1 <= depth <= L + 1
    temb = m.time_embed(timestep, sample.shape[0])
    x = m.conv_in(sample)
    skips = [x]
    last = m.up_blocks[-1]
    if feat is None:
        for blk in m.down_blocks:
            x, outs = blk(x, temb, ehs, cak)
            skips += outs
        if ctrl is not None:
            skips = [s + r for s, r in zip(skips, ctrl)]
        x = m.mid_block(x, temb, ehs, cak)
        if mid_res is not None:
            x = x + mid_res
        for blk in m.up_blocks[:-1]:
            x = blk(x, skips, temb, ehs, cak)
        first = 0
    else:
        for j in range(depth - 1):
            x = _layer(m.down_blocks[0], j, x, temb, ehs, cak)
            skips.append(x)
        if ctrl is not None:
            assert len(ctrl) >= depth
            skips = [s + r for s, r in zip(skips, ctrl)]
        x = feat
        first = L + 1 - depth
    assert not last.add_up
    for j in range(first, L + 1):
        if j == L + 1 - depth:
            feat = x
        x = _layer(last, j, torch.cat([x, skips.pop()], dim=1), temb, ehs, cak)
    assert not skips
    return m.conv_out(F.silu(m.conv_norm_out(x))), feat


def controlnet_forward(m, sample, timestep, ehs, cond, scale=1.0, depth=None):
    """``depth`` None: the full forward; else the shallow one -> (the first ``depth`` residuals, None)"""
    if depth is None:
        return m(sample, timestep, ehs, cond, scale)
    temb = m.time_embed(timestep, sample.shape[0])
    x = m.conv_in(sample) + m.controlnet_cond_embedding(cond)
    skips = [x]
    for j in range(depth - 1):
        x = _layer(m.down_blocks[0], j, x, temb, ehs, {})
        skips.append(x)
    return [zc(s) * scale for s, zc in zip(skips, m.controlnet_down_blocks)], None


class DeepCacheUNet:
    """callable with the oracle UNet's signature; call n belongs to stream n % streams and is that stream's call n // streams"""

    def __init__(self, unet, cache_interval, depth, n_calls, streams=2):
        self.unet, self.depth, self.streams = unet, depth, streams
        self.plan = deepcache_plan(n_calls, cache_interval)
        self.n = 0
        self.feat = [None] * streams
        self.modes = []

    @property
    def attn_processors(self):
        return self.unet.attn_processors

    def __call__(self, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None,
                 down_block_additional_residuals=None, mid_block_additional_residual=None):
        stream, call = self.n % self.streams, self.n // self.streams
        self.n += 1
        full = self.plan[call]
        self.modes.append(full)
        assert full or self.feat[stream] is not None
        eps, feat = unet_forward(self.unet, sample, timestep, encoder_hidden_states, cross_attention_kwargs,
                                 down_block_additional_residuals, mid_block_additional_residual, self.depth,
                                 None if full else self.feat[stream])
        if full:
            self.feat[stream] = feat
        return eps


class DeepCacheControlNet:
    """callable with the oracle ControlNet's signature.  A shallow call returns ``depth`` residuals and (None, None) for the mid
    residual: the oracle loop indexes it by CFG half before handing it to the UNet, which ignores it on a shallow call."""

    def __init__(self, controlnet, cache_interval, depth, n_calls):
        self.controlnet, self.depth = controlnet, depth
        self.plan = deepcache_plan(n_calls, cache_interval)
        self.n = 0

    def __call__(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0):
        full = self.plan[self.n]
        self.n += 1
        if full:
            return controlnet_forward(self.controlnet, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale)
        down, _ = controlnet_forward(self.controlnet, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale,
                                     self.depth)
        return down, (None, None)
