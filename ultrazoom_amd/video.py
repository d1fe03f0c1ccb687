"""8-bit 4:2:0 video frames on the MI355X: YCbCr planes to RGB and back (`mz_yuv420_to_rgb`, `mz_rgb_to_yuv420`: include/mewzoom_hip.h)
behind a tensor interface, and `MewZoom.upscale_yuv420`; below them the same for 10, 12 and 16 bits, 4:2:2, 4:4:4 and BT.2020
(`ycbcr_to_rgb`, `rgb_to_ycbcr`, `frame_planes`, `MewZoom.upscale_ycbcr`).

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


# ---- 8, 10, 12 and 16 bits; 4:2:0, 4:2:2 and 4:4:4; BT.2020 (`mz_ycbcr_to_rgb`, `mz_rgb_to_ycbcr`; ultrazoom_amd/csrc/mz_ycbcr.h) ----------
#
#   * depth: 8 (uint8 planes), 10, 12 or 16 (uint16 planes).  Limited range scales with the depth (Y 16 s..235 s, s = 2^(depth - 8)),
#     full range is 0..2^depth - 1;
#   * align: where a code lies in a uint16 -- "low" (the low bits: yuv420p10le and its kin) or "high" (the high bits, the low ones zero:
#     P010, P012, P016);
#   * subsampling: "420", "422" (chroma [B, 1, H, ceil(W / 2)], no vertical filter) or "444" (chroma [B, 1, H, W], no filter);
#   * matrix: also "bt2020" (Kr = 0.2627, Kb = 0.0593, non-constant luminance).
# With depth 8, "420" and "bt601" / "bt709" the results have the bits of yuv420_to_rgb / rgb_to_yuv420.


def _ycbcr_chroma_shape(B: int, H: int, W: int, subsampling: str):
    return (B, 1, (H + 1) // 2 if subsampling == "420" else H, W if subsampling == "444" else (W + 1) // 2)


def _sample_dtype(depth: int):
    return torch.uint8 if depth == 8 else torch.uint16


def _plane_depth(y, depth) -> int:
    """The depth of planes of y's dtype: `depth`, or 8 for uint8 when it is None."""
    if not isinstance(y, Tensor) or y.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"the planes hold uint8 or uint16 code values, got {y.dtype if isinstance(y, Tensor) else type(y).__name__}")
    if depth is None:
        if y.dtype == torch.uint16:
            raise ValueError("uint16 planes: say depth=10, 12 or 16")
        return 8
    if depth not in _ffi.MZ_YCBCR_DEPTHS:
        raise ValueError(f"depth is 8, 10, 12 or 16, got {depth!r}")
    if _sample_dtype(depth) != y.dtype:
        raise ValueError(f"depth {depth} is held in {_sample_dtype(depth)} planes, got {y.dtype}")
    return depth


def _check_ycbcr_planes(y: Tensor, cb: Tensor, cr: Tensor, depth: int, subsampling: str, want=None):
    """_check_planes for planes of `depth` bits and a subsampling."""
    for name, t in (("y", y), ("cb", cb), ("cr", cr)):
        if not isinstance(t, Tensor) or t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{name} should be a [B, 1, h, w] tensor, got {tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}")
        if t.dtype != _sample_dtype(depth):
            raise ValueError(f"{name} should hold {_sample_dtype(depth)} code values of depth {depth}, got {t.dtype}")
    B, _, H, W = y.shape if want is None else (want[0], 1, want[1], want[2])
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"an empty batch or frame: {tuple(y.shape)}")
    if tuple(y.shape) != (B, 1, H, W):
        raise ValueError(f"y has shape {tuple(y.shape)}, expected {(B, 1, H, W)}")
    shape = _ycbcr_chroma_shape(B, H, W, subsampling)
    for name, t in (("cb", cb), ("cr", cr)):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape} for a {H} x {W} frame in {subsampling}")
    return B, H, W


@torch.inference_mode()
def ycbcr_to_rgb(y: Tensor, cb: Tensor, cr: Tensor, *, depth: Optional[int] = None, align: str = "low", subsampling: str = "420",
                 dtype=torch.float32, matrix: str = "bt709", range: str = "limited", siting: str = "left", clamp: bool = True,
                 out: Optional[Tensor] = None) -> Tensor:
    """`yuv420_to_rgb` for planes of `depth` bits (uint8: 8, the default; uint16: 10, 12 or 16 -- say which), aligned "low" or "high" in
    their uint16, subsampled "420", "422" or "444", with matrix "bt601", "bt709" or "bt2020".  The result, `dtype`, `clamp` and `out` are
    those of `yuv420_to_rgb`."""
    depth = _plane_depth(y, depth)
    fmt, codes = _ffi.ycbcr_codes(depth, align, subsampling, matrix, range, siting)
    B, H, W = _check_ycbcr_planes(y, cb, cr, depth, subsampling)
    if out is not None:
        if out.dim() != 4 or tuple(out.shape) != (B, 3, H, W):
            raise ValueError(f"out has shape {tuple(out.shape)}, expected {(B, 3, H, W)}")
        dtype = out.dtype
    try:
        elem = _ffi.elem_code(dtype)
    except TypeError as e:
        raise ValueError(str(e)) from None
    _check_devices("ycbcr_to_rgb", y, cb, cr, *(() if out is None else (out,)))
    with _ffi.image_frame(y) as (_, _, stream):
        if out is None:
            out = torch.empty((B, 3, H, W), dtype=dtype, device=y.device)
        _ffi.ycbcr_to_rgb(_ffi.pair(y), _ffi.pair(cb), _ffi.pair(cr), *fmt, _ffi.pair(out), elem, B, H, W, *codes, clamp, stream)
    return out


@torch.inference_mode()
def rgb_to_ycbcr(x: Tensor, *, depth: int = 8, align: str = "low", subsampling: str = "420", matrix: str = "bt709", range: str = "limited",
                 siting: str = "left", out: Optional[Planes] = None) -> Planes:
    """`rgb_to_yuv420` into planes of `depth` bits (uint8 for 8, uint16 for 10, 12 and 16), aligned "low" or "high" ("high": the low
    16 - depth bits are written as zeros), subsampled "420", "422" or "444": new dense tensors, or the triple `out`, whose dtype must fit
    `depth` (`frame_planes(buffer, H, W, ...)` writes a frame buffer in place).  Codes are clamped to 0..2^depth - 1."""
    fmt, codes = _ffi.ycbcr_codes(depth, align, subsampling, matrix, range, siting)
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
            raise ValueError("out is a triple (y, cb, cr) of uint8 or uint16 tensors")
        y, cb, cr = out
        _check_ycbcr_planes(y, cb, cr, depth, subsampling, want=(B, H, W))
    _check_devices("rgb_to_ycbcr", x, *(() if out is None else out))
    with _ffi.image_frame(x) as (_, _, stream):
        if out is None:
            y = torch.empty((B, 1, H, W), dtype=_sample_dtype(depth), device=x.device)
            cb, cr = (torch.empty(_ycbcr_chroma_shape(B, H, W, subsampling), dtype=_sample_dtype(depth), device=x.device) for _ in "br")
        _ffi.rgb_to_ycbcr(_ffi.pair(x), elem, _ffi.pair(y), _ffi.pair(cb), _ffi.pair(cr), *fmt, B, H, W, *codes, stream)
    return y, cb, cr


def frame_planes(buffer: Tensor, H: int, W: int, *, layout: str = "semiplanar", order: str = "uv", subsampling: str = "420") -> Planes:
    """The (y, cb, cr) views of a [B, n] uint8 or uint16 buffer of H x W frames, each dense from its first element (n at least the frame's
    element count; any image stride): H * W elements of Y, then the chroma -- `layout="semiplanar"`: Hc rows of Wc interleaved pairs, Cb
    first (`order="uv"`: NV12, P010, P016, NV16, NV24) or Cr first (`"vu"`: NV21, NV61, NV42); `"planar"`: the Hc x Wc Cb plane, then Cr
    (`"uv"`: I420, I422, I444 and their 10 / 12 / 16-bit forms) or Cr before Cb (`"vu"`: YV12, YV16, YV24).  H and W must be even where
    the subsampling halves them.  Nothing is copied."""
    if layout not in ("semiplanar", "planar"):
        raise ValueError(f"layout is 'semiplanar' or 'planar', got {layout!r}")
    cb_first = _order(order)
    if subsampling not in _ffi.MZ_YCBCR_SUBSAMPLINGS:
        raise ValueError(f"subsampling is '420', '422' or '444', got {subsampling!r}")
    if not isinstance(buffer, Tensor) or buffer.dim() != 2 or buffer.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("frame_planes takes a uint8 or uint16 [B, n] buffer of frames")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or (subsampling == "420" and H % 2) or (subsampling != "444" and W % 2):
        raise ValueError(f"a {H} x {W} frame in {subsampling}: H and W are at least 1 and even where the subsampling halves them")
    B, n = buffer.shape
    _, _, hc, wc = _ycbcr_chroma_shape(B, H, W, subsampling)
    if B < 1 or n < H * W + 2 * hc * wc or (n > 1 and buffer.stride(1) != 1):
        raise ValueError(f"a buffer of {B} x {n} elements (strides {tuple(buffer.stride())}) is too short or not dense for {H} x {W} frames "
                         f"in {subsampling}: {H * W + 2 * hc * wc} elements each")
    sb, at = buffer.stride(0), buffer.storage_offset()
    y = buffer.as_strided((B, 1, H, W), (sb, H * W, W, 1), at)
    if layout == "semiplanar":
        first, second = (buffer.as_strided((B, 1, hc, wc), (sb, 2 * hc * wc, 2 * wc, 2), at + H * W + k) for k in (0, 1))
    else:
        first, second = (buffer.as_strided((B, 1, hc, wc), (sb, hc * wc, wc, 1), at + H * W + k * hc * wc) for k in (0, 1))
    return (y,) + ((first, second) if cb_first else (second, first))


@torch.inference_mode()
def upscale_ycbcr(model, y: Tensor, cb: Tensor, cr: Tensor, *, depth: Optional[int] = None, align: str = "low", subsampling: str = "420",
                  matrix: str = "bt709", range: str = "limited", siting: str = "left", out: Optional[Planes] = None) -> Planes:
    """`MewZoom.upscale_ycbcr`: the planes of `model.upscale` of the frames, r times the size, in the depth, alignment and subsampling of
    those that went in -- three calls, no copy between them: `ycbcr_to_rgb` into the dtype of the model's parameters, clamped;
    `model.upscale`; `rgb_to_ycbcr` into `out`.  The intermediate RGB has the MODEL's dtype: a bfloat16 model carries about 8 significant
    bits through, so the low bits of a 10-bit result mean something only with a float16 or float32 model."""
    depth = _plane_depth(y, depth)
    kw = dict(depth=depth, align=align, subsampling=subsampling, matrix=matrix, range=range, siting=siting)
    rgb = ycbcr_to_rgb(y, cb, cr, dtype=next(model.parameters()).dtype, clamp=True, **kw)
    return rgb_to_ycbcr(model.upscale(rgb), out=out, **kw)
