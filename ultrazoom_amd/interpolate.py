"""Plain interpolation of image batches to any size on the MI355X: `mz_interpolate` (include/mewzoom_hip.h) behind a tensor interface.

The arithmetic is that of torch's `interpolate(x, size, mode="nearest" | "bilinear" | "bicubic", align_corners=False)` WITHOUT
antialiasing (its float64 CPU result is the checker of the kernel) -- the model's own skip connection, `Upsample(scale_factor=r,
mode="bicubic")`, and the bicubic baseline the reference's validate.py puts next to every result.  `ultrazoom_amd.resize` is a different
function: antialiased, with the PIL constant A = -0.5.  It runs in HIP on the tensors as they lie in memory: any strides (channels-last, an
HWC frame permuted to NCHW, a crop, every second image), float32 / bfloat16 / float16 / uint8 (a uint8 value v means v / 255 and is stored
as clamp -> * 255 + 0.5 -> truncate).  Bilinear and bicubic accumulate in float64 and round once; nearest moves bit patterns.  Nothing is
copied and nothing here synchronises with the host."""

from __future__ import annotations

from typing import Optional, Tuple

from torch import Tensor

from . import _ffi

_MODES = {"nearest": _ffi.MZ_INTERP_NEAREST, "bilinear": _ffi.MZ_INTERP_BILINEAR, "bicubic": _ffi.MZ_INTERP_BICUBIC}


def interpolate(x: Tensor, size: Optional[Tuple[int, int]] = None, scale_factor: Optional[int] = None, *, mode: str = "bicubic",
                clamp: bool = False, out: Optional[Tensor] = None, window: Optional[Tuple[int, int, int, int]] = None) -> Tensor:
    """A logical [B, 3, H, W] CUDA tensor interpolated to `size` = (Hout, Wout), or enlarged by the positive integer `scale_factor` (then
    size = (H r, W r), where torch's two coordinate rules coincide; any other factor needs `size`); returns a new dense NCHW tensor of x's
    dtype, or `out`.

    `mode` is "nearest" (torch's legacy rule), "bilinear" or "bicubic" (A = -0.75).  `clamp` clamps floating-point results to [0, 1]
    (bicubic overshoots; uint8 results are always clamped; nearest changes no element and takes no clamp).  `window` = (y0, x0, h, w) in
    pixels of the Hout x Wout result selects the part that is computed and stored, `out` ([B, 3, h, w], or [B, 3, Hout, Wout] without a
    window; any strides, x's dtype) receives it in place: a window of a result equals that part of the whole result bit for bit.  Any
    sizes, up or down.  x and out must not overlap."""
    if mode not in _MODES:
        raise ValueError(f"mode is 'nearest', 'bilinear' or 'bicubic', got {mode!r}")
    if clamp and mode == "nearest":
        raise ValueError("nearest moves elements and never changes them: it takes no clamp")
    if (size is None) == (scale_factor is None):
        raise ValueError("give exactly one of size and scale_factor")
    if scale_factor is not None and (isinstance(scale_factor, bool) or not isinstance(scale_factor, int) or scale_factor < 1):
        raise ValueError(f"scale_factor is a positive integer, got {scale_factor!r}: state any other target as size=(Hout, Wout)")
    elem, B, H, W = _ffi.check_image_batch(x, "interpolate")
    if scale_factor is not None:
        size = (H * scale_factor, W * scale_factor)
    Hout, Wout, window, want = _ffi.output_shape(B, size, window)
    with _ffi.image_frame(x, out, want) as (out, _, stream):
        _ffi.interpolate(*_ffi.pair(x), *_ffi.pair(out), elem, B, H, W, Hout, Wout, _MODES[mode], clamp, window, stream)
    return out
