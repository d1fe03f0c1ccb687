"""Antialiased resampling of image batches to any size on the MI355X: `mz_resize` (include/mewzoom_hip.h) behind a tensor interface.

The arithmetic is that of torch's `interpolate(x, size, mode="bicubic" | "bilinear", antialias=True)` (align_corners=False;
its float64 CPU result is the checker of the kernel), in HIP, on the tensors as they lie in memory: any strides (channels-last, an HWC
frame permuted to NCHW, a crop, every second image), float32 / bfloat16 / float16 / uint8 (a uint8 value v means v / 255 and is stored
as clamp -> * 255 + 0.5 -> truncate, as `MewZoom.upscale_uint8` does).  Both passes accumulate in float64; the intermediate between them is float32.  Nothing is copied and
nothing here synchronises with the host."""

from __future__ import annotations

from typing import Optional, Tuple

from torch import Tensor

from . import _ffi

MAX_RATIO = 16  # an axis shrinks at most this much in one call (include/mewzoom_hip.h)


def resize(x: Tensor, size: Tuple[int, int], *, filter: str = "bicubic", clamp: bool = False, out: Optional[Tensor] = None,
           window: Optional[Tuple[int, int, int, int]] = None) -> Tensor:
    """A logical [B, 3, H, W] CUDA tensor resampled to `size` = (Hout, Wout); returns a new dense NCHW tensor of x's dtype, or `out`.

    `clamp` clamps floating-point results to [0, 1] (bicubic overshoots; uint8 results are always clamped).  `window` = (y0, x0, h, w) in
    pixels of the Hout x Wout result selects the part that is computed and stored, `out` ([B, 3, h, w], or [B, 3, Hout, Wout] without a
    window; any strides, x's dtype) receives it in place: a window of a result equals that part of the whole result bit for bit.  An
    axis may shrink by at most 16; enlarging is not bounded.  x and out must not overlap."""
    code = _ffi.resize_filter(filter)
    elem, B, H, W = _ffi.check_image_batch(x, "resize")

    def ratio_check(Hout, Wout):
        if H > MAX_RATIO * Hout or W > MAX_RATIO * Wout:
            raise ValueError(f"{(H, W)} -> {(Hout, Wout)} shrinks an axis by more than {MAX_RATIO}: resize in two steps")

    Hout, Wout, window, want = _ffi.output_shape(B, size, window, ratio_check)
    with _ffi.image_frame(x, out, want, lambda: _ffi.resize_workspace_bytes(H, W, Hout, Wout, code)) as (out, ws, stream):
        _ffi.resize(*_ffi.pair(x), *_ffi.pair(out), elem, B, H, W, Hout, Wout, code, clamp, window, *ws, stream)
    return out
