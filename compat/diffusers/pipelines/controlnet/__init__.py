"""``from diffusers.pipelines.controlnet import MultiControlNetModel``: several ControlNets on one pipeline (imagdressing_amd/unet.py)."""
from imagdressing_amd.unet import MultiControlNetModel  # noqa: F401

__all__ = ["MultiControlNetModel"]
