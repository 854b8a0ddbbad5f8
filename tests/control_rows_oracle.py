"""The ControlNet gate of one request, stated on the oracle (TEST INFRASTRUCTURE): ``oracle.pipeline.denoise`` calls its ControlNet once
per step with one ``conditioning_scale``; diffusers multiplies that by ``controlnet_keep[i]``, 1 inside the request's guidance window
and 0 outside (pipeline_controlnet.py, ``controlnet_keep`` and ``cond_scale = controlnet_conditioning_scale * controlnet_keep[i]``).
The wrapper counts the calls and applies the gate of its call index, so the unmodified oracle loop runs a windowed request."""
from typing import List


def keep(num_steps: int, start: float, end: float) -> List[float]:
    """diffusers: keeps.append(1.0 - float(i / len(timesteps) < s or (i + 1) / len(timesteps) > e))"""
    return [1.0 - float(i / num_steps < start or (i + 1) / num_steps > end) for i in range(num_steps)]


class GatedControlNet:
    """``controlnet(sample, t, ehs, cond, scale)`` -> the wrapped oracle ControlNet at ``scale * keep[call index]``"""

    def __init__(self, controlnet, num_steps: int, start: float = 0.0, end: float = 1.0):
        self.controlnet, self.keep, self.calls = controlnet, keep(num_steps, start, end), 0

    def __call__(self, sample, t, encoder_hidden_states, cond, conditioning_scale=1.0):
        k = self.keep[self.calls]
        self.calls += 1
        return self.controlnet(sample, t, encoder_hidden_states, cond, conditioning_scale * k)
