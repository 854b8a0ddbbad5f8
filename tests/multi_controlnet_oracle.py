"""Several ControlNets of one request, stated on the oracle (TEST INFRASTRUCTURE): ``oracle.pipeline.denoise`` calls its ControlNet once
per step with one control image and one ``conditioning_scale``; diffusers' ``MultiControlNetModel`` runs every net on its own image at
its own ``scale * controlnet_keep[i]`` and sums the residuals (multicontrolnet.py: ``down_samples + down_block_res_samples``).  The
wrapper does that with one ``GatedControlNet`` per net, so the unmodified oracle loop runs a multi-net request; ``second_controlnet``
builds the (oracle, engine) pair of a further net from its own seed, as ``tests.harness.build_pair`` builds the first."""
from tests.control_rows_oracle import GatedControlNet


class SummedControlNets:
    """``controlnet(sample, t, ehs, cond, scale)`` -> the sum over the nets of net k on ``images[k]`` at ``scales[k] * keep_k[call]``
    (``cond`` and ``scale`` of the caller are not read: every net has its own)"""

    def __init__(self, controlnets, images, scales, num_steps: int, starts=None, ends=None):
        K = len(controlnets)
        starts, ends = starts or [0.0] * K, ends or [1.0] * K
        assert len(images) == len(scales) == len(starts) == len(ends) == K
        self.nets = [GatedControlNet(c, num_steps, a, b) for c, a, b in zip(controlnets, starts, ends)]
        self.images, self.scales, self.calls = list(images), [float(s) for s in scales], 0

    def __call__(self, sample, t, encoder_hidden_states, cond=None, conditioning_scale=1.0):
        self.calls += 1
        down = mid = None
        for net, image, s in zip(self.nets, self.images, self.scales):
            d, m = net(sample, t, encoder_hidden_states, image, s)
            down, mid = (list(d), m) if down is None else ([x + y for x, y in zip(down, d)], mid + m)
        return down, mid


def second_controlnet(cfg, seed: int, dtype, device="cuda"):
    """-> (oracle ControlNet, engine ControlNet) with identical weights from ``seed``"""
    from imagdressing_amd import unet as E
    from oracle import sd15
    from tests.harness import oracle_cfg
    sd = E.random_state_dict(E.controlnet_param_shapes(dict(E.SD15_CONFIG, **cfg)), seed, zero_convs=True)
    o = sd15.ControlNetModel(oracle_cfg(cfg))
    o.load_state_dict(sd, strict=True)
    return o, E.ControlNetModel(sd, cfg, device, dtype)
