"""gelslim_depth_amd -- MI355X-native U-Net train/inference step of MMintLab/gelslim_depth.

Importing the package does not load the HIP library (so CPU-only tooling can import `synth`);
`gelslim_depth_amd.models.unet`, `.engine` and `.train` do, and fail loudly if it is missing.
The names of `touch_fusion` are exported lazily: the first use of one imports that module, and with it the library.
"""
_TOUCH_FUSION = ("TouchVolume", "TouchSurface", "touch_transforms", "integrate_touches", "extract_surface", "write_stl")
__all__ = ["synth", *_TOUCH_FUSION]


def __getattr__(name):
    if name in _TOUCH_FUSION:
        from . import touch_fusion
        return getattr(touch_fusion, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
