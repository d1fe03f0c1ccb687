"""Exact-arithmetic reference of the 4:2:0 YCbCr entries (tests/test_yuv_cpu.py, tests/test_yuv_gpu.py, tests/test_poison_yuv_gpu.py):
ultrazoom_amd/csrc/mz_yuv.h restated in Python from the header alone -- nothing here calls the library.  Needs no GPU.

  coeffs            the constants of a matrix and a range: Python-float operations, as the header writes them
  rgb_pixel         YCbCr -> RGB of arrays of pixels: Y codes and UPSAMPLED chroma in code units -> unrounded float64 R, G, B
  yuv_pixel, code   RGB -> YCbCr of arrays of pixels: unrounded float64 y, pb, pr; a code value of scale * v + off
  chroma_up         the upsampling filter of a siting: a chroma plane -> float64 code units at every luma position
  chroma_down       the subsampling filter of a siting: a full-size float64 plane -> the chroma plane's float64 values
  to_rgb_expected   the tensor mz_yuv420_to_rgb stores (the rounding: color_ref.store, luma_round_raw of mz_color.h)
  to_yuv_expected   the three planes mz_rgb_to_yuv420 stores
  SHAPES, planes    the cases of the GPU test and their inputs, every one chosen from the reference alone (seeds)"""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

import color_ref
from image_exact import F64, fma64

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}  # Kr, Kb
RANGES = {"limited": (16.0, 219.0, 224.0), "full": (0.0, 255.0, 255.0)}  # Yoff, Sy, Sc
MATRIX_CODE, RANGE_CODE, SITING_CODE = {"bt601": 0, "bt709": 1}, {"limited": 0, "full": 1}, {"left": 0, "center": 1}
SITINGS = ("left", "center")
# (H, W): one pixel; one row / column / block; odd sides; a row below, at and above one 16-byte run; two runs; a ragged third; several
# workgroups (18 x 258: 306 work items of YCbCr -> RGB)
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (2, 15), (2, 16), (2, 17), (4, 32), (5, 33), (7, 129), (18, 258)]


def coeffs(matrix: str, range_: str) -> dict:
    kr, kb = MATRICES[matrix]
    yoff, sy, sc = RANGES[range_]
    kg = (1.0 - kr) - kb
    a_r, a_b = 2.0 * (1.0 - kr), 2.0 * (1.0 - kb)
    return dict(kr=kr, kg=kg, kb=kb, yoff=yoff, sy=sy, sc=sc, inv_sy=1.0 / sy, inv_sc=1.0 / sc, a_r=a_r, a_b=a_b, g_r=-(kr * a_r) / kg,
                g_b=-(kb * a_b) / kg, pb_scale=0.5 / (1.0 - kb), pr_scale=0.5 / (1.0 - kr))


def debug_coeffs(matrix: str, range_: str):
    """what mz_debug_yuv_coeffs returns: Yoff, 1/Sy, 1/Sc, a_r, a_b, g_r, g_b, Sy, Sc"""
    k = coeffs(matrix, range_)
    return [k[n] for n in ("yoff", "inv_sy", "inv_sc", "a_r", "a_b", "g_r", "g_b", "sy", "sc")]


# ---- per pixel ---------------------------------------------------------------------------------------------------------------------------
def rgb_pixel(k: dict, y, cb, cr):
    """Y codes and upsampled chroma (code units, float64; every value a multiple of 1/16) -> unrounded (R, G, B)"""
    y, cb, cr = (np.asarray(v, dtype=F64) for v in (y, cb, cr))
    yn = (y - k["yoff"]) * k["inv_sy"]
    cbn, crn = (cb - 128.0) * k["inv_sc"], (cr - 128.0) * k["inv_sc"]
    return fma64(k["a_r"], crn, yn), fma64(k["g_b"], cbn, fma64(k["g_r"], crn, yn)), fma64(k["a_b"], cbn, yn)


def yuv_pixel(k: dict, r, g, b):
    """float64 R, G, B -> unrounded (y, pb, pr)"""
    r, g, b = (np.asarray(v, dtype=F64) for v in (r, g, b))
    with np.errstate(all="ignore"):
        y = fma64(k["kb"], b, fma64(k["kg"], g, fma64(k["kr"], r, 0.0)))
        return y, (b - y) * k["pb_scale"], (r - y) * k["pr_scale"]


def code(scale: float, v, off: float) -> np.ndarray:
    """fma(scale, v, off), clamped to [0, 255] (fmin(fmax(.)): a NaN becomes 0), + 0.5, truncated"""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(fma64(scale, v, off), 0.0), 255.0)
        return (c + 0.5).astype(np.uint8)


# ---- the chroma filters --------------------------------------------------------------------------------------------------------------------
def _up_taps(n: int, nc: int, rule: str):
    """(index, neighbour index, weight of the sample, weight of the neighbour) of every position 0..n-1 of one axis"""
    x = np.arange(n)
    i = x >> 1
    if rule == "quarter":  # vertical always, horizontal "center"
        return i, np.clip(np.where(x % 2 == 0, i - 1, i + 1), 0, nc - 1), 0.75, np.full(n, 0.25)
    return i, np.minimum(i + 1, nc - 1), np.where(x % 2 == 0, 1.0, 0.5), np.where(x % 2 == 0, 0.0, 0.5)  # horizontal "left"


def chroma_up(c, H: int, W: int, siting: str) -> np.ndarray:
    """[.., Hc, Wc] codes -> [.., H, W] float64 code units: vertically, then horizontally (every operation is exact)"""
    c = np.asarray(c, dtype=F64)
    j, jn, w0, w1 = _up_taps(H, c.shape[-2], "quarter")
    v = w0 * c[..., j, :] + w1[:, None] * c[..., jn, :]
    i, inb, w0, w1 = _up_taps(W, c.shape[-1], "quarter" if siting == "center" else "left")
    return w0 * v[..., i] + w1 * v[..., inb]


def chroma_down(p, siting: str) -> np.ndarray:
    """[.., H, W] float64 -> [.., Hc, Wc] float64: vertically first, then the taps of the siting, the sums in the header's order"""
    p = np.asarray(p, dtype=F64)
    H, W = p.shape[-2:]
    with np.errstate(all="ignore"):
        rows = np.arange(0, H, 2)
        u = 0.5 * p[..., rows, :] + 0.5 * p[..., np.minimum(rows + 1, H - 1), :]
        cols = np.arange(0, W, 2)
        right = u[..., np.minimum(cols + 1, W - 1)]
        if siting == "center":
            return 0.5 * u[..., cols] + 0.5 * right
        return (0.25 * u[..., np.maximum(cols - 1, 0)] + 0.5 * u[..., cols]) + 0.25 * right


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------
def to_rgb_f64(y, cb, cr, matrix: str, range_: str, siting: str) -> np.ndarray:
    """uint8 planes [B,1,H,W], [B,1,Hc,Wc] twice -> unrounded float64 [B,3,H,W]"""
    y, cb, cr = (np.asarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for t in (y, cb, cr))
    H, W = y.shape[-2:]
    r, g, b = rgb_pixel(coeffs(matrix, range_), y, chroma_up(cb, H, W, siting), chroma_up(cr, H, W, siting))
    return np.concatenate([r, g, b], axis=1)


def to_rgb_expected(y, cb, cr, matrix: str, range_: str, siting: str, dt: str, clamp: int) -> torch.Tensor:
    return color_ref.store(to_rgb_f64(y, cb, cr, matrix, range_, siting), dt, clamp)


def to_yuv_expected(x: torch.Tensor, matrix: str, range_: str, siting: str):
    """[B,3,H,W] of any of the four dtypes -> the uint8 planes (y, cb, cr)"""
    k = coeffs(matrix, range_)
    v = color_ref.values(x)
    y, pb, pr = yuv_pixel(k, v[:, 0:1], v[:, 1:2], v[:, 2:3])
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in
                 (code(k["sy"], y, k["yoff"]), code(k["sc"], chroma_down(pb, siting), 128.0), code(k["sc"], chroma_down(pr, siting), 128.0)))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def chroma_hw(H: int, W: int):
    return (H + 1) // 2, (W + 1) // 2


@lru_cache(maxsize=None)
def planes(B: int, H: int, W: int, seed: int = 3):
    """(y, cb, cr) uint8 on the CPU, built once and left unchanged by their users: every plane is all 256 codes in a shuffled order, as far
    as it has room, then noise"""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    out = []
    for shape in ((B, 1, H, W), (B, 1) + chroma_hw(H, W), (B, 1) + chroma_hw(H, W)):
        n = B * shape[2] * shape[3]
        t = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64)
        m = min(n, 256)
        t[:m] = torch.randperm(256, generator=g)[:m]
        out.append(t[torch.randperm(n, generator=g)].to(torch.uint8).reshape(shape))
    return tuple(out)


@lru_cache(maxsize=None)
def rgb_f64(B: int, H: int, W: int, matrix: str, range_: str, siting: str) -> np.ndarray:
    """the unrounded reference of `planes`, computed once"""
    return to_rgb_f64(*planes(B, H, W), matrix, range_, siting)


@lru_cache(maxsize=None)
def yuv_of_image(B: int, H: int, W: int, dt: str, matrix: str, range_: str, siting: str):
    """the reference planes of color_ref.image(B, H, W, dt), computed once"""
    return to_yuv_expected(color_ref.image(B, H, W, dt), matrix, range_, siting)


def grey_chroma_frames(B: int, H: int, W: int, seed: int = 11):
    """frames with random Y and chroma constant per image (the round-trip test: such chroma survives both filters exactly)"""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    y = torch.randint(0, 256, (B, 1, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    hc, wc = chroma_hw(H, W)
    cb, cr = (torch.randint(0, 256, (B, 1, 1, 1), generator=g, dtype=torch.int64).to(torch.uint8).expand(B, 1, hc, wc).contiguous() for _ in "br")
    return y, cb, cr
