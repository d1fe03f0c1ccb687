"""Exact-arithmetic reference of the YCbCr entries of any depth and subsampling (tests/test_ycbcr_cpu.py, tests/test_ycbcr_gpu.py,
tests/test_poison_ycbcr_gpu.py): ultrazoom_amd/csrc/mz_ycbcr.h restated in Python from the header alone -- nothing here calls the
library.  Needs no GPU.  What the header takes from mz_yuv.h is taken from tests/yuv_ref.py.

  coeffs             the constants of a matrix, a range and a depth: Python-float operations, as the header writes them
  read, write        a code of a stored word and back (depth, align)
  rgb_pixel, code    per pixel: Y codes and UPSAMPLED chroma in code units -> unrounded R, G, B; a code value of scale * v + off
  chroma_up, _down   the filters of a subsampling and a siting
  to_rgb_expected    the tensor mz_ycbcr_to_rgb stores (the rounding: color_ref.store)
  to_ycbcr_expected  the three planes mz_rgb_to_ycbcr stores
  FORMATS, planes    the cases of the GPU tests and their inputs, every one chosen from the reference alone (seeds)"""

from __future__ import annotations

import itertools
from functools import lru_cache

import numpy as np
import torch

import color_ref
import yuv_ref
from image_exact import F64, fma64

DEPTHS = (8, 10, 12, 16)
ALIGNS = ("low", "high")
SUBSAMPLINGS = ("420", "422", "444")
MATRICES = dict(yuv_ref.MATRICES, bt2020=(0.2627, 0.0593))  # Kr, Kb
MATRIX_CODE = {"bt601": 0, "bt709": 1, "bt2020": 2}
RANGE_CODE, SITING_CODE, SITINGS = yuv_ref.RANGE_CODE, yuv_ref.SITING_CODE, yuv_ref.SITINGS
ALIGN_CODE, SUB_CODE = {"low": 0, "high": 1}, {"420": 0, "422": 1, "444": 2}
SHAPES = yuv_ref.SHAPES


def coeffs(matrix: str, range_: str, depth: int) -> dict:
    kr, kb = MATRICES[matrix]
    s, maxc, mid = float(2 ** (depth - 8)), float(2 ** depth - 1), float(2 ** (depth - 1))
    yoff, sy, sc = (0.0, maxc, maxc) if range_ == "full" else (16.0 * s, 219.0 * s, 224.0 * s)
    kg = (1.0 - kr) - kb
    a_r, a_b = 2.0 * (1.0 - kr), 2.0 * (1.0 - kb)
    return dict(kr=kr, kg=kg, kb=kb, yoff=yoff, sy=sy, sc=sc, inv_sy=1.0 / sy, inv_sc=1.0 / sc, a_r=a_r, a_b=a_b, g_r=-(kr * a_r) / kg,
                g_b=-(kb * a_b) / kg, pb_scale=0.5 / (1.0 - kb), pr_scale=0.5 / (1.0 - kr), mid=mid, maxc=maxc)


def debug_coeffs(matrix: str, range_: str, depth: int):
    """what mz_debug_ycbcr_coeffs returns: Yoff, 1/Sy, 1/Sc, a_r, a_b, g_r, g_b, Sy, Sc, mid, max code"""
    k = coeffs(matrix, range_, depth)
    return [k[n] for n in ("yoff", "inv_sy", "inv_sc", "a_r", "a_b", "g_r", "g_b", "sy", "sc", "mid", "maxc")]


# ---- words and codes ---------------------------------------------------------------------------------------------------------------------
def sample_dtype(depth: int):
    return np.uint8 if depth == 8 else np.uint16


def shift_of(depth: int, align: str) -> int:
    return 16 - depth if align == "high" and depth > 8 else 0


def read(words, depth: int, align: str) -> np.ndarray:
    """(word >> shift) & (2^d - 1): "high" ignores the low bits, "low" the high ones"""
    return (np.asarray(words).astype(np.int64) >> shift_of(depth, align)) & (2 ** depth - 1)


def write(codes, depth: int, align: str) -> np.ndarray:
    return (np.asarray(codes).astype(np.int64) << shift_of(depth, align)).astype(sample_dtype(depth))


def as_numpy(t) -> np.ndarray:
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---- per pixel ---------------------------------------------------------------------------------------------------------------------------
def rgb_pixel(k: dict, y, cb, cr):
    """Y codes and upsampled chroma (code units, float64; every value a multiple of 1/16) -> unrounded (R, G, B)"""
    y, cb, cr = (np.asarray(v, dtype=F64) for v in (y, cb, cr))
    yn = (y - k["yoff"]) * k["inv_sy"]
    scale = k["inv_sc"] * 0.0625
    cbn, crn = (16.0 * cb - 16.0 * k["mid"]) * scale, (16.0 * cr - 16.0 * k["mid"]) * scale
    return fma64(k["a_r"], crn, yn), fma64(k["g_b"], cbn, fma64(k["g_r"], crn, yn)), fma64(k["a_b"], cbn, yn)


def code(scale: float, v, off: float, maxc: float) -> np.ndarray:
    """fma(scale, v, off), clamped to [0, 2^d - 1] (fmin(fmax(.)): a NaN becomes 0), + 0.5, truncated"""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(fma64(scale, v, off), 0.0), maxc)
        return (c + 0.5).astype(np.int64)


# ---- the chroma filters --------------------------------------------------------------------------------------------------------------------
def chroma_hw(H: int, W: int, sub: str):
    return ((H + 1) // 2 if sub == "420" else H), (W if sub == "444" else (W + 1) // 2)


def chroma_up(c, H: int, W: int, siting: str, sub: str) -> np.ndarray:
    """[.., Hc, Wc] codes -> [.., H, W] float64 code units (every operation is exact)"""
    c = np.asarray(c, dtype=F64)
    if sub == "420":
        return yuv_ref.chroma_up(c, H, W, siting)
    if sub == "444":
        return c
    i, inb, w0, w1 = yuv_ref._up_taps(W, c.shape[-1], "quarter" if siting == "center" else "left")  # 4:2:2: the horizontal rule alone
    return w0 * c[..., i] + w1 * c[..., inb]


def chroma_down(p, siting: str, sub: str) -> np.ndarray:
    """[.., H, W] float64 -> [.., Hc, Wc] float64"""
    p = np.asarray(p, dtype=F64)
    if sub == "420":
        return yuv_ref.chroma_down(p, siting)
    if sub == "444":
        return p
    W = p.shape[-1]
    with np.errstate(all="ignore"):
        cols = np.arange(0, W, 2)
        right = p[..., np.minimum(cols + 1, W - 1)]
        if siting == "center":
            return 0.5 * p[..., cols] + 0.5 * right
        return (0.25 * p[..., np.maximum(cols - 1, 0)] + 0.5 * p[..., cols]) + 0.25 * right


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------
def to_rgb_f64(y, cb, cr, depth: int, align: str, sub: str, matrix: str, range_: str, siting: str) -> np.ndarray:
    """planes of stored words [B,1,H,W], [B,1,Hc,Wc] twice -> unrounded float64 [B,3,H,W]"""
    y, cb, cr = (read(as_numpy(t), depth, align) for t in (y, cb, cr))
    H, W = y.shape[-2:]
    r, g, b = rgb_pixel(coeffs(matrix, range_, depth), y, chroma_up(cb, H, W, siting, sub), chroma_up(cr, H, W, siting, sub))
    return np.concatenate([r, g, b], axis=1)


def to_rgb_expected(y, cb, cr, depth, align, sub, matrix, range_, siting, dt: str, clamp: int) -> torch.Tensor:
    return color_ref.store(to_rgb_f64(y, cb, cr, depth, align, sub, matrix, range_, siting), dt, clamp)


def to_ycbcr_expected(x: torch.Tensor, depth: int, align: str, sub: str, matrix: str, range_: str, siting: str):
    """[B,3,H,W] of any of the four dtypes -> the planes (y, cb, cr) of stored words, numpy uint8 / uint16"""
    k = coeffs(matrix, range_, depth)
    v = color_ref.values(x)
    y, pb, pr = yuv_ref.yuv_pixel(k, v[:, 0:1], v[:, 1:2], v[:, 2:3])
    codes = (code(k["sy"], y, k["yoff"], k["maxc"]), code(k["sc"], chroma_down(pb, siting, sub), k["mid"], k["maxc"]),
             code(k["sc"], chroma_down(pr, siting, sub), k["mid"], k["maxc"]))
    return tuple(np.ascontiguousarray(write(c, depth, align)) for c in codes)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _signed(t: torch.Tensor) -> torch.Tensor:
    """uint16 data under the int16 view of the same bits: what every copy kernel of torch takes"""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def tensor(a: np.ndarray, device="cpu") -> torch.Tensor:
    """a uint8 / uint16 array as a tensor of the same dtype"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(device).view(torch.uint16)
    return torch.from_numpy(a).to(device)


def put(view: torch.Tensor, src) -> None:
    """view[...] = src (an array, or a tensor on any device) for uint8 and uint16 alike"""
    src = src if isinstance(src, torch.Tensor) else tensor(src)
    _signed(view).copy_(_signed(src).to(view.device))


def words(t: torch.Tensor) -> np.ndarray:
    """the stored words of a plane on any device, any strides"""
    a = _signed(t).cpu().numpy()
    return a.view(np.uint16) if t.dtype == torch.uint16 else a


def same_words(got: torch.Tensor, want: np.ndarray) -> bool:
    g = words(got)
    return g.dtype == want.dtype and g.shape == want.shape and bool(np.array_equal(g, want))


@lru_cache(maxsize=None)
def planes(B: int, H: int, W: int, depth: int, sub: str, seed: int = 3):
    """(y, cb, cr) of stored WORDS, numpy, built once and left unchanged: every bit of a word is random -- the bits a format does not
    read (the low 16 - d of "high", the high ones of "low") hold garbage; the first words are 0, all ones, and the extreme codes of both
    alignments"""
    rng = np.random.default_rng(seed + 1000 * H + W + 7 * depth)
    hc, wc = chroma_hw(H, W, sub)
    top = 256 if depth == 8 else 65536
    special = [0, top - 1, (2 ** depth - 1) % top, ((2 ** depth - 1) << (16 - depth)) % top if depth > 8 else 255, 2 ** (depth - 1)]
    out = []
    for shape in ((B, 1, H, W), (B, 1, hc, wc), (B, 1, hc, wc)):
        a = rng.integers(0, top, size=shape, dtype=np.int64)
        flat = a.reshape(-1)
        flat[: min(len(special), flat.size)] = special[: flat.size]
        out.append(rng.permutation(flat).reshape(shape).astype(sample_dtype(depth)))
    return tuple(out)


@lru_cache(maxsize=None)
def rgb_f64(B, H, W, depth, align, sub, matrix, range_, siting) -> np.ndarray:
    """the unrounded reference of `planes`, computed once"""
    return to_rgb_f64(*planes(B, H, W, depth, sub), depth, align, sub, matrix, range_, siting)


@lru_cache(maxsize=None)
def ycbcr_of_image(B, H, W, dt, depth, align, sub, matrix, range_, siting):
    """the reference planes of color_ref.image(B, H, W, dt), computed once"""
    return to_ycbcr_expected(color_ref.image(B, H, W, dt), depth, align, sub, matrix, range_, siting)


def grey_chroma_frames(B: int, H: int, W: int, depth: int, align: str, sub: str, seed: int = 11):
    """frames of stored words with random Y codes and chroma constant per image (the round-trip test: such chroma survives every
    filter exactly); the bits the format does not hold are zero, as a writer leaves them"""
    rng = np.random.default_rng(seed + 1000 * H + W + depth)
    hc, wc = chroma_hw(H, W, sub)
    y = rng.integers(0, 2 ** depth, size=(B, 1, H, W), dtype=np.int64)
    cb, cr = (np.broadcast_to(rng.integers(0, 2 ** depth, size=(B, 1, 1, 1), dtype=np.int64), (B, 1, hc, wc)) for _ in "br")
    return tuple(np.ascontiguousarray(write(a, depth, align)) for a in (y, cb, cr))


# The cases of the GPU tests: every (depth, align, subsampling), the other parameters cycled over them (all 3 x 2 x 2 x 2 combinations of
# matrix, range, siting and clamp occur)
FORMATS = [(d, a, s) for d in DEPTHS for a in ALIGNS for s in SUBSAMPLINGS]
PARAMS = list(itertools.product(sorted(MATRIX_CODE), sorted(RANGE_CODE), SITINGS, (1, 0)))


def params_of(index: int, n: int = 2):
    """n of PARAMS for case `index`, walking the list"""
    return [PARAMS[(index * n + t) % len(PARAMS)] for t in range(n)]
