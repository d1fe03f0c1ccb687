"""The luma (Y) plane of RGB image batches on the MI355X: `mz_luma` (include/mewzoom_hip.h) behind a tensor interface.

Super-resolution papers and leaderboards report PSNR and SSIM on the Y channel of BT.601 YCbCr.  Two standards:
  * "bt601": studio range, MATLAB's `rgb2ycbcr` and basicsr's `bgr2ycbcr(y_only=True)`:
    Y = 16/255 + (65.481 R + 128.553 G + 24.966 B) / 255 for R, G, B in [0, 1]; white is 235/255, black 16/255;
  * "full": full range, BT.601 / JFIF / Pillow's "L": Y = 0.299 R + 0.587 G + 0.114 B.
The sum is float64 (three fused multiply-adds, `ultrazoom_amd/csrc/mz_color.h`) and rounded once to the tensor's dtype.  It runs in HIP
on the tensors as they lie in memory: any strides (channels-last, BGR through a flipped channel axis, a crop, every second image, a grey
image broadcast with channel stride 0), float32 / bfloat16 / float16 / uint8 (a uint8 value v means v / 255 and is stored as clamp ->
* 255 + 0.5 -> truncate).  Nothing is copied and nothing here synchronises with the host.

`ultrazoom_amd.metrics.image_metrics(..., luma="bt601")` measures on the UNROUNDED float64 Y planes.  MATLAB's variant, which rounds Y
to uint8 first, is this function on uint8 images, broadcast back to three equal channels (a read view may have stride 0):

    image_metrics(rgb_to_y(p).expand(-1, 3, -1, -1), rgb_to_y(t).expand(-1, 3, -1, -1))
"""

from __future__ import annotations

from typing import Optional

from torch import Tensor

from . import _ffi


def rgb_to_y(x: Tensor, standard: str = "bt601", *, clamp: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """The Y plane [B, 1, H, W] of a logical [B, 3, H, W] CUDA tensor (channels in R, G, B order), of x's dtype: a new dense tensor, or
    `out` (any strides).  `clamp` clamps floating-point results to [0, 1] (uint8 results are always clamped).  x and out must not overlap."""
    code = _ffi.luma_standard(standard)
    elem, B, H, W = _ffi.check_image_batch(x, "rgb_to_y")
    with _ffi.image_frame(x, out, (B, 1, H, W)) as (out, _, stream):
        _ffi.luma(*_ffi.pair(x), *_ffi.pair(out), elem, B, H, W, code, clamp, stream)
    return out
