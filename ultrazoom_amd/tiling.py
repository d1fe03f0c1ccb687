"""Exact image-level tiling for inputs whose activations do not fit in HBM (BASELINE configs[4] is the
"tiled single-image" case).  The reference has no tiling code: this is host-side slicing around `MewZoom.upscale`.

Why it is exact.  Every output pixel depends on a bounded window of the input (3x3 convolutions at four resolutions,
2x2 stride-2 PixelCrush, PixelShuffle, the 4-tap bicubic skip): `receptive_field(config)` low-resolution pixels on
each side.  A tile is upscaled together with a halo of at least that many pixels and only its core is kept, so what
the zero padding / index clamping at an artificial cut changes never reaches a kept pixel.  Tile origins are
multiples of 8 so that the three stride-2 levels, their floors at odd sizes and the decoder's bottom/right zero
padding (model.py:650-689) fall on the same pixels as in the whole image; cuts at the true image border keep the
true border.  The kernels accumulate in an order that does not depend on where a pixel sits in its tensor, so
tiled and untiled results agree bit for bit, and the tiled fp32 result meets the reference's fixtures (tests/test_tiling.py).

Feathered tiling (`plan_feathered`, `upscale_feathered`, `feather_paste`) is the other mode: tiles cut with a SMALL halo, which no longer
agree where they meet, each kept `overlap` pixels beyond every interior cut and cross-faded over that band by `mz_feather_paste`
(include/mewzoom_hip.h; ultrazoom_amd/csrc/mz_feather.h states the arithmetic).  It is not exact -- a tile sees only `halo` pixels of
context -- unless the halo covers the receptive field plus the overlap, where every kept pixel is the untiled one and the paste, a
select wherever two tiles agree, changes no bit.  `tile_work` is the price of either mode: slice pixels per image pixel."""

from __future__ import annotations

import math
from collections import namedtuple
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _ffi


def receptive_field(config: dict) -> int:
    """Upper bound of the one-sided receptive field of `upscale` in low-resolution pixels, rounded up to a multiple
    of 8 (block counts per stage as model.py:277-300: ceil(L/2) encoder + floor(L/2) decoder blocks of two 3x3
    convolutions each)."""
    layers = [config[f"{n}_layers"] for n in ("primary", "secondary", "tertiary", "quaternary")]
    r = 0.0
    for s, L in enumerate(layers):
        blocks = math.ceil(L / 2) + L // 2
        r += 2 * blocks * 2**s          # two 3x3 convolutions per block, one pixel of that level each
    r += sum(2**s for s in (1, 2, 3))   # the 3x3 of each decoder sub-pixel convolution (runs at the coarser level)
    r += sum(2 ** (s - 1) for s in (1, 2, 3))  # PixelCrush 2x2 / stride 2: up to one pixel of the finer level
    for i in range(int(math.log2(config["upscale_ratio"]))):
        r += 3 * 2.0**-i                # head stage i: refiner block (2 convs) + sub-pixel conv at 2^i x resolution
    r += 2                              # bicubic skip: 4 taps
    return int(math.ceil(r / 8.0)) * 8 + 8


@torch.inference_mode()
def upscale_tiled(model, x: Tensor, tile: Tuple[int, int] = (512, 512), halo: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """`model.upscale(x)` computed tile by tile.  `tile` = core size in low-resolution pixels (rounded up to multiples
    of 8); `halo` defaults to `receptive_field(config)`; a smaller halo is refused, because the result would no
    longer equal the untiled one.

    A model that offers `upscale_into` (MewZoom) gets one call per tile with the haloed slice of `x` as an input view,
    the tile's core as the output window and the core's place in the result as the output view: no slice is copied, no
    haloed tile is written anywhere, and uint8 input gives `model.upscale_uint8(x)`.  Any other object with `upscale`
    is called on contiguous slices and the cores are copied out, as before.

    `out` ([B, 3, rH, rW], any strides, x's dtype and device) receives the result in place of a new tensor (`upscale_ensemble` passes
    its one pass scratch)."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("expected a [B, 3, H, W] tensor")
    cfg = model._cfg
    need = receptive_field(cfg)
    halo = need if halo is None else int(halo)
    if halo < need or halo % 8:
        raise ValueError(f"halo must be a multiple of 8 and at least the receptive field ({need} pixels), got {halo}")
    th, tw = (max(8, (int(t) + 7) // 8 * 8) for t in tile)
    B, _, H, W = x.shape
    r = cfg["upscale_ratio"]
    if out is None:
        out = torch.empty((B, 3, H * r, W * r), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (B, 3, H * r, W * r) or out.dtype != x.dtype or out.device != x.device:
        raise ValueError(f"out should be a {(B, 3, H * r, W * r)} {x.dtype} tensor on {x.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    into = getattr(model, "upscale_into", None)
    for y0 in range(0, H, th):
        y1 = min(H, y0 + th)
        ya, yb = max(0, y0 - halo), min(H, y1 + halo)
        for x0 in range(0, W, tw):
            x1 = min(W, x0 + tw)
            xa, xb = max(0, x0 - halo), min(W, x1 + halo)
            core = out[:, :, y0 * r : y1 * r, x0 * r : x1 * r]
            if into is not None:
                into(x[:, :, ya:yb, xa:xb], core, window=((y0 - ya) * r, (x0 - xa) * r, (y1 - y0) * r, (x1 - x0) * r))
                continue
            sr = model.upscale(x[:, :, ya:yb, xa:xb].contiguous())
            core.copy_(sr[:, :, (y0 - ya) * r : (y1 - ya) * r, (x0 - xa) * r : (x1 - xa) * r])
    return out


# ---- feathered tiling --------------------------------------------------------------------------------------------------------------
Rect = namedtuple("Rect", "y0 x0 y1 x1")             # rows [y0, y1), columns [x0, x1), in low-resolution pixels
FeatherTile = namedtuple("FeatherTile", "core slice kept")


def _tile_sides(tile) -> Tuple[int, int]:
    th, tw = (max(8, (int(t) + 7) // 8 * 8) for t in tile)
    return th, tw


def _axis(n: int, t: int, halo: int, overlap: int):
    """(core, slice, kept) intervals of the tiles of one axis of n pixels"""
    out = []
    for c0 in range(0, n, t):
        c1 = min(n, c0 + t)
        kept = (c0 - overlap if c0 > 0 else 0, min(n, c1 + overlap) if c1 < n else n)  # beyond a cut only: a side with a neighbour
        out.append(((c0, c1), (max(0, c0 - halo), min(n, c1 + halo)), kept))
    return out


def plan_feathered(H: int, W: int, tile: Tuple[int, int], halo: int, overlap: int) -> List[List[FeatherTile]]:
    """The tiles of an H x W image as rows of `FeatherTile(core, slice, kept)`, each a `Rect(y0, x0, y1, x1)` in low-resolution pixels.
    A pure function.

    core:  the cores partition the image; `tile` is rounded up to multiples of 8, so their origins are multiples of 8.
    slice: what the model is given -- the core plus `halo` on every side, clipped to the image.
    kept:  what is kept of the result -- the core plus `overlap` on every side that has a neighbour, clipped to the image.  Around an
           interior cut at c the two neighbours' kept parts share the band [c - overlap, c + overlap), cut short by the image's end
           where the last core is narrower than the overlap.

    `halo` is a multiple of 8 (slices begin on multiples of 8, as cores do) and at least 0; 0 <= overlap <= halo (a kept pixel lies in
    its slice); 2 * overlap <= min(th, tw), which keeps the bands of two cuts apart.  Anything else is a ValueError."""
    H, W, halo, overlap = int(H), int(W), int(halo), int(overlap)
    if H < 1 or W < 1:
        raise ValueError(f"an empty image: {H} x {W}")
    th, tw = _tile_sides(tile)
    if halo < 0 or halo % 8:
        raise ValueError(f"halo must be a multiple of 8 and at least 0, got {halo}")
    if not 0 <= overlap <= halo:
        raise ValueError(f"overlap must lie in [0, halo = {halo}], got {overlap}")
    if 2 * overlap > min(th, tw):
        raise ValueError(f"overlap = {overlap} is more than half a {th} x {tw} tile: the bands of two cuts would meet")
    return [[FeatherTile(Rect(cy[0], cx[0], cy[1], cx[1]), Rect(sy[0], sx[0], sy[1], sx[1]), Rect(ky[0], kx[0], ky[1], kx[1]))
             for cx, sx, kx in _axis(W, tw, halo, overlap)] for cy, sy, ky in _axis(H, th, halo, overlap)]


def tile_work(H: int, W: int, tile: Tuple[int, int], halo: int) -> float:
    """Slice pixels divided by image pixels: the arithmetic of a tiling with this core size and halo, in units of the untiled image's."""
    area = sum((t.slice.y1 - t.slice.y0) * (t.slice.x1 - t.slice.x0) for row in plan_feathered(H, W, tile, halo, 0) for t in row)
    return area / (int(H) * int(W))


def feather_paste(src: Tensor, dst: Tensor, ramp: Tuple[int, int] = (0, 0)) -> Tensor:
    """`src` pasted onto `dst` (two logical [B, 3, H, W] CUDA tensors of one dtype -- float32 / bfloat16 / float16 / uint8 -- with any
    strides, not overlapping) with a linear cross-fade of `ramp` = (ny, nx) positions from the top and the left edge: `mz_feather_paste`.
    Position k of a ramp of n gives src the weight (2 k + 1) / (2 n); an element's weight is the product of its row's and its column's.
    Outside both ramps dst receives src bit for bit and is not read; inside, d + w (s - d) in float64, rounded once.  Returns dst."""
    elem, B, H, W = _ffi.check_image_batch(src, "feather_paste", dst, ("src", "dst"))
    ny, nx = (int(v) for v in ramp)
    with torch.cuda.device(src.device):
        _ffi.feather_paste(_ffi.pair(src), _ffi.pair(dst), elem, B, H, W, ny, nx, torch.cuda.current_stream(src.device).cuda_stream)
    return dst


@torch.inference_mode()
def upscale_feathered(model, x: Tensor, tile: Tuple[int, int] = (512, 512), halo: int = 32, overlap: Optional[int] = None,
                      out: Optional[Tensor] = None) -> Tensor:
    """`model.upscale(x)` (`upscale_uint8` for uint8 tensors) approximated tile by tile with a small halo, the seams cross-faded.
    `plan_feathered(H, W, tile, halo, overlap)` names the tiles; `overlap` defaults to `halo // 2`.  With r the model's ratio and
    n = 2 * overlap * r, the order of operations -- it fixes the bits -- is:

      * every tile result is `model.upscale_into(slice of x, dst, window = kept relative to slice)` (an object without `upscale_into`:
        `upscale` of the contiguous slice, the kept part copied out);
      * tile row j is assembled left to right in a strip (the row's kept rows, all columns): the first tile is written by the model
        straight into the strip, every later one into a tile scratch and pasted onto its kept columns of the strip with ramp_x = n;
      * strip 0 is the top rows of `out` itself; every later strip lies in a strip scratch and is pasted onto its kept rows of `out`
        with ramp_y = n.

    `overlap = 0` is the hard cut: every core is written straight into `out`, no paste, no scratch.  A halo of at least
    `receptive_field(config) + overlap` gives `upscale(x)` bit for bit.  `out` ([B, 3, rH, rW], any strides, x's dtype and device)
    receives the result in place.  Nothing here synchronises with the host; memory beyond `out`: one kept tile and one strip."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("expected a [B, 3, H, W] tensor")
    r = model._cfg["upscale_ratio"]
    halo = int(halo)
    overlap = halo // 2 if overlap is None else int(overlap)
    B, _, H, W = x.shape
    rows = plan_feathered(H, W, tile, halo, overlap)
    if out is None:
        out = torch.empty((B, 3, H * r, W * r), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (B, 3, H * r, W * r) or out.dtype != x.dtype or out.device != x.device:
        raise ValueError(f"out should be a {(B, 3, H * r, W * r)} {x.dtype} tensor on {x.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    into = getattr(model, "upscale_into", None)

    def run(t: FeatherTile, dst: Tensor) -> None:  # dst = the kept part of the tile's result
        s, k = t.slice, t.kept
        xs = x[:, :, s.y0 : s.y1, s.x0 : s.x1]
        if into is not None:
            into(xs, dst, window=((k.y0 - s.y0) * r, (k.x0 - s.x0) * r, (k.y1 - k.y0) * r, (k.x1 - k.x0) * r))
        else:
            sr = model.upscale(xs.contiguous())
            dst.copy_(sr[:, :, (k.y0 - s.y0) * r : (k.y1 - s.y0) * r, (k.x0 - s.x0) * r : (k.x1 - s.x0) * r])

    def rows_of(k: Rect) -> Tensor:
        return out[:, :, k.y0 * r : k.y1 * r, :]

    if overlap == 0:
        for row in rows:
            for t in row:
                run(t, rows_of(t.kept)[:, :, :, t.kept.x0 * r : t.kept.x1 * r])
        return out

    def scratch(h: int, w: int) -> Tensor:  # rows 16 bytes aligned in every dtype: the paste's 16-byte path
        return torch.empty((B, 3, h, (w + 15) // 16 * 16), dtype=x.dtype, device=x.device)

    n = 2 * overlap * r
    kept_h = [(row[0].kept.y1 - row[0].kept.y0) * r for row in rows]
    kept_w = [(t.kept.x1 - t.kept.x0) * r for t in rows[0]]
    tile_buf = scratch(max(kept_h), max(kept_w[1:])) if len(kept_w) > 1 else None
    strip_buf = scratch(max(kept_h[1:]), W * r) if len(kept_h) > 1 else None
    for j, row in enumerate(rows):
        strip = rows_of(row[0].kept) if j == 0 else strip_buf[:, :, : kept_h[j], : W * r]
        for i, t in enumerate(row):
            cols = strip[:, :, :, t.kept.x0 * r : t.kept.x1 * r]
            if i == 0:
                run(t, cols)
            else:
                mine = tile_buf[:, :, : kept_h[j], : kept_w[i]]
                run(t, mine)
                feather_paste(mine, cols, ramp=(0, n))
        if j > 0:
            feather_paste(strip, rows_of(row[0].kept), ramp=(n, 0))
    return out
