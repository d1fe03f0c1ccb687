"""8-bit 4:2:0 video frames on the MI355X: YCbCr planes to RGB and back (`mz_yuv420_to_rgb`, `mz_rgb_to_yuv420`: include/mewzoom_hip.h)
behind a tensor interface, and `MewZoom.upscale_yuv420`.

Video decoders and encoders exchange 8-bit 4:2:0 YCbCr: a full-size Y plane and Cb, Cr planes of half the size in both directions,
uint8 CODE VALUES 0..255.  The planes are three tensors: y [B, 1, H, W], cb and cr [B, 1, ceil(H / 2), ceil(W / 2)], with ANY strides.
A container layout is a choice of views, not of kernels -- `nv12_planes` (NV12 / NV21: Cb and Cr interleaved behind Y) and
`i420_planes` (I420 / YV12: two planar chroma planes behind Y) cut the three views out of a frame buffer without copying, and the views
serve as inputs and as `out=`.

  * matrix: "bt601" (Kr = 0.299, Kb = 0.114) or "bt709" (Kr = 0.2126, Kb = 0.0722);
  * range: "limited" (Y 16..235, chroma 16..240) or "full" (0..255);
  * siting: "left" (a chroma sample sits on luma column 2i, between luma rows 2j and 2j + 1: MPEG-2, H.264, HEVC) or "center" (in the
    middle of its 2 x 2 luma block: JPEG, MPEG-1).

The arithmetic (`ultrazoom_amd/csrc/mz_yuv.h` states it once) is float64 with sums in a fixed order and one rounding on store; chroma is
upsampled with the 3/4, 1/4 taps of its siting and subsampled with the matching 1/2, 1/2 (center) or 1/4, 1/2, 1/4 (left) taps over
the unrounded colour differences.  Odd H and W are legal: indices clamp at the edges.  Nothing here synchronises with the host.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _ffi

Planes = Tuple[Tensor, Tensor, Tensor]


def _chroma_shape(B: int, H: int, W: int):
    return (B, 1, (H + 1) // 2, (W + 1) // 2)


def _check_devices(what: str, first: Tensor, *others: Tensor) -> None:
    """Every tensor of a call is on one CUDA device (after the call's ValueErrors)."""
    if not first.is_cuda:
        raise RuntimeError(f"ultrazoom_amd.{what} computes on an MI355X only: move the tensors to a 'cuda' device. There is no CPU path.")
    for t in others:
        if t.device != first.device:
            raise RuntimeError(f"ultrazoom_amd.{what}: tensors on {first.device} and on {t.device}")


def _check_planes(y: Tensor, cb: Tensor, cr: Tensor, want=None):
    """(B, H, W) of three uint8 planes, from shapes and dtypes alone; `want`: the (B, H, W) they must have (the `out` of rgb_to_yuv420)."""
    for name, t in (("y", y), ("cb", cb), ("cr", cr)):
        if not isinstance(t, Tensor) or t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{name} should be a [B, 1, h, w] tensor, got {tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
        if t.dtype != torch.uint8:
            raise ValueError(f"{name} should hold uint8 code values, got {t.dtype}")
    B, _, H, W = y.shape if want is None else (want[0], 1, want[1], want[2])
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"an empty batch or frame: {tuple(y.shape)}")
    if tuple(y.shape) != (B, 1, H, W):
        raise ValueError(f"y has shape {tuple(y.shape)}, expected {(B, 1, H, W)}")
    for name, t in (("cb", cb), ("cr", cr)):
        if tuple(t.shape) != _chroma_shape(B, H, W):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {_chroma_shape(B, H, W)} for a {H} x {W} frame")
    return B, H, W


@torch.inference_mode()
def yuv420_to_rgb(y: Tensor, cb: Tensor, cr: Tensor, *, dtype=torch.float32, matrix: str = "bt709", range: str = "limited",
                  siting: str = "left", clamp: bool = True, out: Optional[Tensor] = None) -> Tensor:
    """RGB [B, 3, H, W] of the uint8 planes y [B, 1, H, W], cb and cr [B, 1, ceil(H / 2), ceil(W / 2)]: a new dense tensor of `dtype`
    (float32, bfloat16, float16 or uint8), or `out` (any strides; its dtype decides).  Floating-point results are in units of [0, 1] and
    clamped to it unless `clamp` is False (out-of-gamut colours and limited-range foot- and headroom then survive); uint8 results are
    always clamped.  `out` must not overlap the planes."""
    codes = _ffi.yuv_codes(matrix, range, siting)
    B, H, W = _check_planes(y, cb, cr)
    if out is not None:
        if out.dim() != 4 or tuple(out.shape) != (B, 3, H, W):
            raise ValueError(f"out has shape {tuple(out.shape)}, expected {(B, 3, H, W)}")
        dtype = out.dtype
    try:
        elem = _ffi.elem_code(dtype)
    except TypeError as e:
        raise ValueError(str(e)) from None
    _check_devices("yuv420_to_rgb", y, cb, cr, *(() if out is None else (out,)))
    with _ffi.image_frame(y) as (_, _, stream):
        if out is None:
            out = torch.empty((B, 3, H, W), dtype=dtype, device=y.device)
        _ffi.yuv420_to_rgb(_ffi.pair(y), _ffi.pair(cb), _ffi.pair(cr), _ffi.pair(out), elem, B, H, W, *codes, clamp, stream)
    return out


@torch.inference_mode()
def rgb_to_yuv420(x: Tensor, *, matrix: str = "bt709", range: str = "limited", siting: str = "left", out: Optional[Planes] = None) -> Planes:
    """The uint8 planes (y [B, 1, H, W], cb, cr [B, 1, ceil(H / 2), ceil(W / 2)]) of a logical [B, 3, H, W] CUDA tensor (R, G, B order;
    float32, bfloat16, float16 in units of [0, 1], or uint8; any strides): new dense tensors, or the triple `out` of uint8 tensors or
    views (any strides: `nv12_planes(buffer)` writes an NV12 frame buffer in place).  Codes are clamped to 0..255, not to the nominal
    range.  x must not overlap the planes; Cb and Cr may interleave with each other and must not overlap otherwise."""
    codes = _ffi.yuv_codes(matrix, range, siting)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected a [B, 3, H, W] tensor, got {tuple(x.shape)}")
    try:
        elem = _ffi.elem_code(x.dtype)
    except TypeError as e:
        raise ValueError(str(e)) from None
    B, _, H, W = x.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"an empty batch or image: {tuple(x.shape)}")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("out is a triple (y, cb, cr) of uint8 tensors")
        y, cb, cr = out
        _check_planes(y, cb, cr, want=(B, H, W))
    _check_devices("rgb_to_yuv420", x, *(() if out is None else out))
    with _ffi.image_frame(x) as (_, _, stream):
        if out is None:
            y = torch.empty((B, 1, H, W), dtype=torch.uint8, device=x.device)
            cb, cr = (torch.empty(_chroma_shape(B, H, W), dtype=torch.uint8, device=x.device) for _ in "br")
        _ffi.rgb_to_yuv420(_ffi.pair(x), elem, _ffi.pair(y), _ffi.pair(cb), _ffi.pair(cr), B, H, W, *codes, stream)
    return y, cb, cr


def _frame_size(frames: Tensor, what: str):
    if not isinstance(frames, Tensor) or frames.dim() != 3 or frames.dtype != torch.uint8:
        raise ValueError(f"{what} takes a uint8 [B, H * 3 / 2, W] frame buffer")
    B, rows, W = frames.shape
    H = rows * 2 // 3
    if B < 1 or rows < 3 or rows % 3 or H % 2 or W < 2 or W % 2:
        raise ValueError(f"{what}: a [B, H * 3 / 2, W] buffer with H and W even, got {tuple(frames.shape)}")
    return B, H, W


def _order(order: str) -> bool:
    if order not in ("uv", "vu"):
        raise ValueError(f"order is 'uv' (Cb first) or 'vu' (Cr first), got {order!r}")
    return order == "uv"


def nv12_planes(frames: Tensor, order: str = "uv") -> Planes:
    """The (y, cb, cr) views of a uint8 [B, H * 3 / 2, W] buffer of NV12 frames (H, W even; any strides): H rows of Y, then H / 2 rows of
    interleaved chroma pairs -- Cb first (`order="uv"`, NV12) or Cr first (`"vu"`, NV21).  Nothing is copied."""
    _, H, W = _frame_size(frames, "nv12_planes")
    pairs = frames[:, H:, :].unflatten(2, (W // 2, 2))  # [B, H / 2, W / 2, 2]
    first, second = pairs[..., 0].unsqueeze(1), pairs[..., 1].unsqueeze(1)
    return (frames[:, :H, :].unsqueeze(1),) + ((first, second) if _order(order) else (second, first))


def i420_planes(frames: Tensor, order: str = "uv") -> Planes:
    """The (y, cb, cr) views of a uint8 [B, H * 3 / 2, W] buffer of I420 frames (H, W even; each frame dense: row stride W, column stride
    1): H rows of Y, then the H / 2 x W / 2 Cb plane, then Cr (`order="uv"`, I420) or Cr before Cb (`"vu"`, YV12).  Nothing is copied."""
    B, H, W = _frame_size(frames, "i420_planes")
    if frames.stride(2) != 1 or frames.stride(1) != W:
        raise ValueError(f"i420_planes: every frame should be dense (strides (.., {W}, 1)), got {tuple(frames.stride())}")
    at, hc, wc = frames.storage_offset() + H * W, H // 2, W // 2
    first, second = (frames.as_strided((B, 1, hc, wc), (frames.stride(0), hc * wc, wc, 1), at + n * hc * wc) for n in (0, 1))
    return (frames[:, :H, :].unsqueeze(1),) + ((first, second) if _order(order) else (second, first))


@torch.inference_mode()
def upscale_yuv420(model, y: Tensor, cb: Tensor, cr: Tensor, *, matrix: str = "bt709", range: str = "limited", siting: str = "left",
                   out: Optional[Planes] = None) -> Planes:
    """`MewZoom.upscale_yuv420`: the planes of `model.upscale` of the frames, r times the size -- three calls, no copy between them:
    `yuv420_to_rgb` into the dtype of the model's parameters, clamped; `model.upscale`; `rgb_to_yuv420` into `out`."""
    rgb = yuv420_to_rgb(y, cb, cr, dtype=next(model.parameters()).dtype, matrix=matrix, range=range, siting=siting, clamp=True)
    return rgb_to_yuv420(model.upscale(rgb), matrix=matrix, range=range, siting=siting, out=out)
