"""``from diffusers.pipelines.controlnet.multicontrolnet import MultiControlNetModel`` (the library's module path of the class)."""
from imagdressing_amd.unet import MultiControlNetModel  # noqa: F401

__all__ = ["MultiControlNetModel"]
