"""MI355X-native implementation of the MewZoom upscale path (andrewdalpino/UltraZoom v0.3.0).

    from ultrazoom_amd import MewZoom          # drop-in for ultrazoom.model.MewZoom
    model = MewZoom.from_pretrained(...).to("cuda").eval()
    y = model.upscale(x)

All arithmetic runs in hand-written gfx950 kernels behind the C ABI in include/mewzoom_hip.h.
"""

from .alpha import alpha_fill, alpha_merge, upscale_rgba  # noqa: F401
from .color import rgb_to_y  # noqa: F401
from .degrade import Degradation, gaussian_blur, gaussian_noise, jpeg  # noqa: F401
from .ensemble import dihedral, dihedral_inverse, upscale_ensemble  # noqa: F401
from .interpolate import interpolate  # noqa: F401
from .model import MewZoom, bake_state_dict  # noqa: F401
from .tiling import feather_paste, upscale_feathered  # noqa: F401
from .video import frame_planes, i420_planes, nv12_planes, rgb_to_ycbcr, rgb_to_yuv420, ycbcr_to_rgb, yuv420_to_rgb  # noqa: F401

__all__ = ["MewZoom", "bake_state_dict", "Degradation", "gaussian_blur", "gaussian_noise", "jpeg", "dihedral", "dihedral_inverse",
           "upscale_ensemble", "interpolate", "rgb_to_y", "yuv420_to_rgb", "rgb_to_yuv420", "nv12_planes", "i420_planes",
           "ycbcr_to_rgb", "rgb_to_ycbcr", "frame_planes", "alpha_fill", "alpha_merge", "upscale_rgba",
           "feather_paste", "upscale_feathered"]
