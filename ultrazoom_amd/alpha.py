"""Images with an alpha channel on the MI355X: `mz_alpha_fill` and `mz_alpha_merge` (include/mewzoom_hip.h) behind a tensor interface,
and `upscale_rgba`, which puts the model between them.

Why.  In a straight-alpha image (a PNG, WebP or TIFF cut-out, a sprite, a logo) the colour under the fully transparent pixels is
arbitrary: black, white, whatever the editor left.  The model's one-sided receptive field is hundreds of low-resolution pixels
(`tiling.receptive_field`), so every visible edge pixel of `upscale(x[:, :3])` pulls that colour in and gets a dark or bright fringe.
`alpha_fill` replaces the colour under a == 0 by the visible colour extrapolated over the WHOLE transparent region (a push-pull pyramid:
2 x 2 weighted sums down to one texel, bilinear enlargement back up), bit for bit independent of what those pixels held; visible pixels
keep their bits.  `alpha_merge` enlarges the alpha plane with the arithmetic of the model's own skip (`ultrazoom_amd.interpolate`) and
premultiplies the colour if asked.  ultrazoom_amd/csrc/mz_alpha.h states the arithmetic; everything runs in HIP on the tensors as they
lie in memory -- any strides (a permuted HWC RGBA array from an image decoder goes in as it is), float32 / bfloat16 / float16 / uint8
(a uint8 value v means v / 255) -- nothing is copied and nothing here synchronises with the host.

Out of scope: grey and grey + alpha images (expand the grey plane to three channels first); alpha through the model (the plane is
interpolated, never inferred); the self-ensemble (`upscale_ensemble` takes RGB); metrics with alpha (`evaluate`, `metrics` take RGB)."""

from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _ffi

_MODES = {"nearest": _ffi.MZ_INTERP_NEAREST, "bilinear": _ffi.MZ_INTERP_BILINEAR, "bicubic": _ffi.MZ_INTERP_BICUBIC}


def _check_plane(rgb: Tensor, alpha: Tensor, B: int) -> None:
    """`alpha` is a [B, 1, h, w] plane on rgb's device and of rgb's dtype"""
    if not isinstance(alpha, Tensor) or alpha.dim() != 4 or alpha.shape[0] != B or alpha.shape[1] != 1 or min(alpha.shape[2:]) < 1:
        raise ValueError(f"alpha should be a [{B}, 1, h, w] tensor, got {tuple(alpha.shape) if isinstance(alpha, Tensor) else type(alpha).__name__}")
    if alpha.device != rgb.device:
        raise RuntimeError(f"the colour is on {rgb.device} but alpha is on {alpha.device}")
    if alpha.dtype != rgb.dtype:
        raise TypeError(f"the colour ({rgb.dtype}) and alpha ({alpha.dtype}) should have the same dtype")


@torch.inference_mode()
def alpha_fill(rgb: Tensor, alpha: Tensor, *, premultiplied: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """The straight colour of a logical [B, 3, H, W] CUDA tensor with the pixels under `alpha` == 0 ([B, 1, H, W], the same dtype; values
    outside [0, 1] are clamped, NaN reads as 0) filled from the visible ones; returns a new dense [B, 3, H, W] tensor, or `out` (any
    strides; it must not overlap the inputs).

    Pixels with alpha > 0 come back bit for bit (`premultiplied=True`: divided by their alpha, clamped to [0, 1], rounded once).  Pixels
    with alpha == 0 get the push-pull extrapolation, which never reads their colour arithmetically: NaN, infinities or noise there change
    no bit of the result.  An image without a visible pixel comes back as zeros.  `rgb` and `alpha` may be `x[:, :3]` and `x[:, 3:4]` of
    one RGBA tensor of any layout."""
    elem, B, H, W = _ffi.check_image_batch(rgb, "alpha_fill")
    _check_plane(rgb, alpha, B)
    if tuple(alpha.shape) != (B, 1, H, W):
        raise ValueError(f"alpha has shape {tuple(alpha.shape)}, expected {(B, 1, H, W)}")
    with _ffi.image_frame(rgb, out, (B, 3, H, W), need=lambda: _ffi.alpha_fill_workspace_bytes(B, H, W)) as (out, ws, stream):
        _ffi.alpha_fill(_ffi.pair(rgb), _ffi.pair(alpha), _ffi.pair(out), elem, B, H, W, premultiplied, *ws, stream)
    return out


def _same_view(a: Tensor, b: Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and tuple(a.stride()) == tuple(b.stride())


@torch.inference_mode()
def alpha_merge(sr: Tensor, alpha: Tensor, *, size: Tuple[int, int], mode: str = "bicubic", premultiply: bool = False,
                out: Optional[Tensor] = None) -> Tensor:
    """The [B, 4, Hout, Wout] RGBA image of the colour `sr` ([B, 3, Hout, Wout]) and the low-resolution plane `alpha` ([B, 1, H, W])
    enlarged to `size` = (Hout, Wout): a new dense tensor, or `out` (any strides, e.g. a permuted [B, Hout, Wout, 4] buffer).

    `out[:, 3:4]` has the bits of `interpolate(alpha.expand(B, 3, H, W), size, mode=mode, clamp=True)[:, :1]` ("nearest" moves elements and
    clamps nothing).  `premultiply=True` stores colour * A, rounded once, with A the alpha element as stored, so the pair is consistent;
    otherwise the colour is stored as it is.  `sr` may be `out[:, :3]` itself: then the colour is premultiplied in place, or not touched
    at all."""
    if mode not in _MODES:
        raise ValueError(f"mode is 'nearest', 'bilinear' or 'bicubic', got {mode!r}")
    elem, B, Hout, Wout = _ffi.check_image_batch(sr, "alpha_merge")
    size = tuple(int(v) for v in size)
    if size != (Hout, Wout):
        raise ValueError(f"size is {size} but the colour is {Hout} x {Wout}")
    _check_plane(sr, alpha, B)
    H, W = alpha.shape[2:]
    if out is not None:
        _ffi.check_same_batch(sr, out, (B, 4, Hout, Wout))
    with _ffi.image_frame(sr) as (_, _, stream):
        if out is None:
            out = torch.empty((B, 4, Hout, Wout), dtype=sr.dtype, device=sr.device)
        rgb_out = out[:, :3]
        if not premultiply and not _same_view(sr, rgb_out):
            rgb_out.copy_(sr)
        pairs = (_ffi.pair(sr), _ffi.pair(rgb_out)) if premultiply else (None, None)
        _ffi.alpha_merge(pairs[0], _ffi.pair(alpha), pairs[1], _ffi.pair(out[:, 3:4]), elem, B, H, W, Hout, Wout, _MODES[mode], premultiply, stream)
    return out


@torch.inference_mode()
def upscale_rgba(model, x: Tensor, *, premultiplied: bool = False, alpha_mode: str = "bicubic", out: Optional[Tensor] = None,
                 tile: Optional[Tuple[int, int]] = None) -> Tensor:
    """`MewZoom.upscale_rgba`: the [B, 4, rH, rW] upscaled RGBA image of `x`, a logical [B, 4, H, W] CUDA tensor with ANY strides -- of
    the dtype of the model's parameters, or uint8 -- as three public calls with no copy between them: `alpha_fill` of `x[:, :3]` under
    `x[:, 3:4]`; `model.upscale_into` of the filled colour straight into `out[:, :3]` (`tiling.upscale_tiled(..., out=out[:, :3])` with
    `tile`); `alpha_merge` of `x[:, 3:4]` into `out[:, 3:4]` by `alpha_mode`.  `premultiplied=True` takes premultiplied colour and gives
    premultiplied colour.  `out` ([B, 4, rH, rW], any strides, x's dtype: a permuted HWC buffer for an image encoder) receives the
    result in place of a new dense tensor.  No host synchronisation beyond `upscale`'s; the pyramid is one `torch.empty`.

    An opaque image gives the bits of `upscale(x[:, :3])` and an alpha of exactly 1.  Out of scope: grey and grey + alpha images, alpha
    through the model, the self-ensemble, metrics with alpha."""
    if not isinstance(x, Tensor) or x.dim() != 4 or x.shape[1] != 4:
        raise ValueError(f"expected a [B, 4, H, W] tensor, got {tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__}")
    B, _, H, W = x.shape
    r = model.upscale_ratio
    want = (B, 4, H * r, W * r)
    if out is None:
        out = torch.empty(want, dtype=x.dtype, device=x.device)
    else:
        _ffi.check_same_batch(x, out, want)
    filled = alpha_fill(x[:, :3], x[:, 3:4], premultiplied=premultiplied)
    if tile is not None:
        from .tiling import upscale_tiled

        upscale_tiled(model, filled, tile=tile, out=out[:, :3])
    else:
        model.upscale_into(filled, out[:, :3])
    return alpha_merge(out[:, :3], x[:, 3:4], size=(H * r, W * r), mode=alpha_mode, premultiply=premultiplied, out=out)
