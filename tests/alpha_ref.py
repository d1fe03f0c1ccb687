"""Exact-arithmetic reference of the alpha entries (tests/test_alpha_cpu.py, tests/test_alpha_gpu.py, tests/test_poison_alpha_gpu.py):
ultrazoom_amd/csrc/mz_alpha.h restated in numpy float64 from the header alone -- nothing here calls the library.  Needs no GPU.

  levels, workspace_bytes   the pyramid: level 0 = H x W, level l + 1 = ceil / 2, down to 1 x 1; the workspace holds levels 1.., 16 bytes
                            a texel, 16 bytes at least
  texels0 / push / pull     the three steps on [B, 4, h, w] float64 arrays that hold float32 values (w, r, g, b)
  fill_expected             the tensor mz_alpha_fill stores
  merge_expected            (out_alpha, out_rgb or None) of mz_alpha_merge: image_exact.interp_expected on the plane, the float64 product
  rgba                      the inputs of the GPU tests: colour noise, alpha with zeros, ones and fractions

Every fma is image_exact.fma64; a stored component is rounded once to float32 (astype); the store of a result is color_ref.store."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

import color_ref
import image_exact
from color_ref import DTYPES, ELEM  # noqa: F401  (the tests take them from here)
from image_exact import F32, F64, clamp01, fma64

SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (9, 8), (17, 33), (64, 48)]
MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}


def levels(H: int, W: int):
    out = [(H, W)]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def workspace_bytes(B: int, H: int, W: int) -> int:
    return max(16, sum(B * h * w * 16 for h, w in levels(H, W)[1:]))


def f32(v: np.ndarray) -> np.ndarray:
    """the one rounding of a stored component"""
    with np.errstate(all="ignore"):
        return np.asarray(v, dtype=F64).astype(F32).astype(F64)


def alpha_values(alpha: torch.Tensor) -> np.ndarray:
    """[B, 1, H, W]: the element by the view's rule, clamped to [0, 1], a NaN as 0"""
    return clamp01(color_ref.values(alpha))


def straight(rgb: torch.Tensor, a: np.ndarray, premultiplied: bool) -> np.ndarray:
    """the straight colour c, [B, 3, H, W] float64 (meaningless under a == 0 for straight input: whatever the elements hold)"""
    v = color_ref.values(rgb)
    if not premultiplied:
        return v
    with np.errstate(all="ignore"):
        return np.where(a > 0, clamp01(v / np.where(a > 0, a, 1.0)), 0.0)


def texels0(a: np.ndarray, c: np.ndarray) -> np.ndarray:
    """level 0: (a, a c) where a > 0, exactly zero elsewhere -- a select"""
    with np.errstate(all="ignore"):
        return np.where(a > 0, f32(np.concatenate([a, a * c], axis=1)), 0.0)


def push(t: np.ndarray) -> np.ndarray:
    B, _, h, w = t.shape
    p = np.zeros((B, 4, h + h % 2, w + w % 2))  # a child that does not exist: the zero texel, which changes no bit of the sums
    p[:, :, :h, :w] = t
    s = np.zeros((B, 4, (h + 1) // 2, (w + 1) // 2))
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        s = s + p[:, :, dy::2, dx::2]
    sw = s[:, 0:1]
    with np.errstate(all="ignore"):
        s = np.where(sw > 1.0, np.concatenate([np.ones_like(sw), s[:, 1:] / np.where(sw > 1.0, sw, 1.0)], axis=1), s)
    return f32(s)


def enlarge(up: np.ndarray, h: int, w: int) -> np.ndarray:
    """U of every texel of an h x w level from the pulled coarser level `up`: unrounded float64"""
    hu, wu = up.shape[2:]
    y, x = np.arange(h), np.arange(w)
    py, px = y >> 1, x >> 1
    ny = np.clip(py + np.where(y & 1, 1, -1), 0, hu - 1)
    nx = np.clip(px + np.where(x & 1, 1, -1), 0, wu - 1)
    acc = np.zeros(up.shape[:2] + (h, w))
    for wt, yy, xx in ((0.5625, py, px), (0.1875, py, nx), (0.1875, ny, px), (0.0625, ny, nx)):
        acc = fma64(wt, up[:, :, yy][:, :, :, xx], acc)
    return acc


def pull(t: np.ndarray, up: np.ndarray) -> np.ndarray:
    U = enlarge(up, t.shape[2], t.shape[3])
    return f32(fma64(1.0 - t[:, 0:1], U, t))


def pulled_level1(a: np.ndarray, c: np.ndarray):
    """level 1 after push and pull, or None for a 1 x 1 image"""
    pyr = [texels0(a, c)]
    while pyr[-1].shape[2:] != (1, 1):
        pyr.append(push(pyr[-1]))
    if len(pyr) == 1:
        return None
    for l in range(len(pyr) - 2, 0, -1):
        pyr[l] = pull(pyr[l], pyr[l + 1])
    return pyr[1]


def fill_expected(rgb: torch.Tensor, alpha: torch.Tensor, dt: str, premultiplied: bool) -> torch.Tensor:
    """rgb [B, 3, H, W], alpha [B, 1, H, W] of dtype `dt` on the CPU -> the [B, 3, H, W] result"""
    assert rgb.dtype == DTYPES[dt] and alpha.dtype == DTYPES[dt]
    a = alpha_values(alpha)
    c = straight(rgb, a, premultiplied)
    H, W = a.shape[2:]
    l1 = pulled_level1(a, c)
    U = enlarge(l1, H, W) if l1 is not None else np.zeros((a.shape[0], 4, H, W))  # texel' of a == 0 pixels: fma(1, U, 0) = U
    with np.errstate(all="ignore"):
        fill = np.where(U[:, 0:1] > 0, clamp01(U[:, 1:] / np.where(U[:, 0:1] > 0, U[:, 0:1], 1.0)), 0.0)
    filled = color_ref.store(fill, dt, 0)
    visible = rgb.cpu() if not premultiplied else color_ref.store(c, dt, 0)
    return torch.where(torch.from_numpy(a > 0), visible, filled)


def merge_expected(sr, alpha: torch.Tensor, size, mode: str, dt: str, premultiply: bool):
    """(out_alpha [B, 1, Hout, Wout], out_rgb or None)"""
    out_alpha = image_exact.interp_expected(alpha.cpu(), size, mode, dt, 0 if mode == "nearest" else 1)
    if not premultiply:
        return out_alpha, None
    with np.errstate(all="ignore"):
        return out_alpha, color_ref.store(color_ref.values(sr) * color_ref.values(out_alpha), dt, 0)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def rgba(B: int, H: int, W: int, dt: str, seed: int = 11, kind: str = "mixed") -> torch.Tensor:
    """[B, 4, H, W] on the CPU, built once and left unchanged by its users.  Colour: noise over [0, 1] (uint8: all bytes).  Alpha, `kind`:
    "mixed" -- about a third zeros, a third ones, a third fractions, different in every image; "binary" -- zeros and ones; "opaque";
    "clear" -- all zero.  Image 1 of a "mixed" batch keeps one visible pixel only, so that whole levels of its pyramid are empty."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    u = torch.rand((B, 4, H, W), generator=g, dtype=torch.float64)
    pick = torch.rand((B, 1, H, W), generator=g, dtype=torch.float64)
    al = u[:, 3:4]
    if kind == "mixed":
        al = torch.where(pick < 1 / 3, torch.zeros_like(al), torch.where(pick < 2 / 3, torch.ones_like(al), al))
        if B > 1:
            al[1] = 0
            al[1, 0, H // 2, W // 3] = 0.75
    elif kind == "binary":
        al = (pick < 0.4).double()
        al[:, :, H // 2, W // 2] = 1.0
    elif kind == "opaque":
        al = torch.ones_like(al)
    else:
        al = torch.zeros_like(al)
    x = torch.cat([u[:, :3], al], dim=1)
    if dt == "u8":
        return (x * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
    return x.to(DTYPES[dt])


def premultiplied_of(x: torch.Tensor, dt: str) -> torch.Tensor:
    """the same batch with its colour multiplied by its alpha, rounded to the type: a premultiplied input"""
    v = color_ref.values(x)
    out = x.clone()
    out[:, :3] = color_ref.store(v[:, :3] * v[:, 3:4], dt, 0)
    return out


def garbage(x: torch.Tensor, dt: str, what: str, seed: int = 3) -> torch.Tensor:
    """x with the colour under every a == 0 pixel replaced: "nan", "inf" (float types; uint8: 255 and 0) or "random" """
    clear = (alpha_values(x[:, 3:4]) == 0)
    out = x.clone()
    if dt == "u8":
        fill = {"nan": 255, "inf": 0}.get(what)
        g = torch.Generator().manual_seed(seed)
        junk = torch.randint(0, 256, x[:, :3].shape, generator=g, dtype=torch.int64).to(torch.uint8) if fill is None else torch.full_like(x[:, :3], fill)
    else:
        g = torch.Generator().manual_seed(seed)
        junk = {"nan": torch.full(x[:, :3].shape, float("nan"), dtype=torch.float64), "inf": torch.full(x[:, :3].shape, float("inf"), dtype=torch.float64)}.get(what)
        if junk is None:
            junk = torch.rand(x[:, :3].shape, generator=g, dtype=torch.float64) * 1e4 - 5e3
        junk = junk.to(DTYPES[dt])
    out[:, :3] = torch.where(torch.from_numpy(clear), junk, x[:, :3])
    return out


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    return color_ref.same_bits(got, want)
