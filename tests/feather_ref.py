"""Exact-arithmetic reference of feathered tiling (tests/test_feather_cpu.py, tests/test_feather_gpu.py, tests/test_poison_feather_gpu.py,
tests/test_far_feather_gpu.py): ultrazoom_amd/csrc/mz_feather.h restated in numpy float64 from the header alone, and the strip order of
ultrazoom_amd.tiling.upscale_feathered given the per-tile results -- nothing here calls the library.  Needs no GPU.

  omega, weights     the ramp weights (2 k + 1) * (1.0 / (2 n)) and the [H, W] products of a paste
  paste_expected     the tensor mz_feather_paste leaves in dst, bit for bit: the select where w == 1 or the bit patterns agree, else
                     d + w (s - d) rounded once (bf16 / f16: image_exact.round64, as alpha_ref.py's stores; uint8: codes, + 0.5, truncate)
  paste_f64          the same on unrounded float64 arrays: the effective weights of a plan
  blend              the strip order: rows left to right into a strip, strips top to bottom onto the result
  pair               the inputs of the GPU tests, with the planted cases"""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

import image_exact
from color_ref import DTYPES, ELEM, TINY  # noqa: F401  (the tests take them from here)
from image_exact import F32, F64

MAX_RAMP = 1 << 20
JUNK = {"f32": float("nan"), "bf16": float("nan"), "f16": float("nan"), "u8": 0xA5}  # what stands for uninitialised memory


def omega(n: int, k) -> np.ndarray:
    """omega(n, k) of integer positions k >= 0"""
    k = np.asarray(k, dtype=np.int64)
    if n == 0:
        return np.ones(k.shape, dtype=F64)
    rho = 1.0 / (2.0 * float(n))
    return np.where(k < n, (2 * k + 1).astype(F64) * rho, 1.0)


def weights(H: int, W: int, ny: int, nx: int) -> np.ndarray:
    """[H, W]: w = omega(ny, y) * omega(nx, x)"""
    return omega(ny, np.arange(H))[:, None] * omega(nx, np.arange(W))[None, :]


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def values(t: torch.Tensor) -> np.ndarray:
    """what the blend takes an element for: the float types' values, uint8 the codes themselves"""
    t = t.cpu()
    return t.numpy().astype(F64) if t.dtype == torch.uint8 else t.double().numpy()


def paste_expected(src: torch.Tensor, dst: torch.Tensor, ramp, dt: str) -> torch.Tensor:
    """src, dst [B, 3, H, W] of dtype `dt` -> what dst holds after the paste (on the CPU)"""
    src, dst = src.cpu(), dst.cpu()
    assert src.dtype == DTYPES[dt] and dst.dtype == DTYPES[dt] and src.shape == dst.shape
    w = weights(src.shape[2], src.shape[3], int(ramp[0]), int(ramp[1]))
    s, d = values(src), values(dst)
    with np.errstate(all="ignore"):
        t = s - d
        p = w * t
        v = d + p
        if dt == "u8":
            blended = torch.from_numpy(np.where(np.isfinite(v), v + 0.5, 0.0).astype(np.int64).astype(np.uint8))
        elif dt == "f32":
            blended = torch.from_numpy(v.astype(F32))
        else:
            blended = image_exact.round64(v, dt)
    take = torch.from_numpy(np.broadcast_to(w == 1.0, s.shape).copy()) | (bits(src) == bits(dst))
    return torch.where(take, src, blended)


def paste_f64(src: np.ndarray, dst: np.ndarray, ramp) -> np.ndarray:
    """the paste on float64 arrays, nothing rounded to an element type"""
    w = weights(src.shape[-2], src.shape[-1], int(ramp[0]), int(ramp[1]))
    with np.errstate(all="ignore"):
        return np.where(w == 1.0, src, dst + w * (src - dst))


def blend(plan, tiles, r: int, overlap: int, paste, out, new_strip):
    """The strip order of upscale_feathered.  plan: plan_feathered's rows; tiles[j][i]: the kept result of tile (j, i), [B, 3, kh r, kw r];
    paste(src, dst, ramp) -> the new dst; out: [B, 3, H r, W r], holding anything; new_strip(h) -> a [B, 3, h, W r] array holding anything.
    Works on torch tensors and numpy arrays alike."""
    n = 2 * overlap * r
    for j, row in enumerate(plan):
        k0 = row[0].kept
        strip = new_strip((k0.y1 - k0.y0) * r)
        for i, t in enumerate(row):
            cols = slice(t.kept.x0 * r, t.kept.x1 * r)
            strip[..., cols] = tiles[j][i] if i == 0 else paste(tiles[j][i], strip[..., cols], (0, n))
        rows = slice(k0.y0 * r, k0.y1 * r)
        out[:, :, rows] = strip if j == 0 else paste(strip, out[:, :, rows], (n, 0))
    return out


def blend_expected(plan, tiles, r: int, overlap: int, dt: str, B: int, H: int, W: int) -> torch.Tensor:
    """the result of upscale_feathered from its tiles' kept results (CPU tensors of dtype `dt`), bit for bit"""
    junk = lambda *shape: torch.full(shape, JUNK[dt], dtype=DTYPES[dt])  # noqa: E731
    return blend(plan, tiles, r, overlap, lambda s, d, ramp: paste_expected(s, d, ramp, dt), junk(B, 3, H * r, W * r),
                 lambda h: junk(B, 3, h, W * r))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def pair(B: int, H: int, W: int, dt: str, ramp, seed: int = 17):
    """(src, dst) on the CPU, built once and left unchanged by their users.  Noise over [0, 1] (uint8: all bytes) with, planted at random:
    elements in which dst equals src bit for bit, a -0 in both among them; subnormals of the type in either; uint8: dst within 1, 2 or 8
    codes of src, where the weights 1/2, 1/4, 3/4 and 1/16 of the tests' ramps land on .5 ties; and NaN (uint8: 0xA5) in dst under every
    second element with w == 1."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W + 7 * int(ramp[0]) + 3 * int(ramp[1]))
    shape = (B, 3, H, W)
    pick = torch.rand(shape, generator=g)
    if dt == "u8":
        src = torch.randint(0, 256, shape, generator=g, dtype=torch.int64)
        dst = torch.randint(0, 256, shape, generator=g, dtype=torch.int64)
        step = torch.tensor([1, 2, 8, -1, -2, -8])[torch.randint(0, 6, shape, generator=g)]
        dst = torch.where(pick < 0.4, (src + step).clamp(0, 255), dst)
        dst = torch.where((pick >= 0.4) & (pick < 0.5), src, dst)
        src, dst = src.to(torch.uint8), dst.to(torch.uint8)
    else:
        src = torch.rand(shape, generator=g, dtype=torch.float64).to(DTYPES[dt])
        dst = torch.rand(shape, generator=g, dtype=torch.float64).to(DTYPES[dt])
        tiny = (torch.randint(-3, 4, shape, generator=g).double() * TINY[dt]).to(DTYPES[dt])
        src = torch.where(pick < 0.1, tiny, src)
        dst = torch.where((pick >= 0.05) & (pick < 0.2), tiny.flip(3), dst)
        same = (pick >= 0.4) & (pick < 0.5)
        src = torch.where(same & (pick < 0.42), torch.tensor(-0.0, dtype=DTYPES[dt]), src)
        dst = torch.where(same, src, dst)
    w1 = torch.from_numpy(np.broadcast_to(weights(H, W, int(ramp[0]), int(ramp[1])) == 1.0, shape).copy())
    dst = torch.where(w1 & (torch.rand(shape, generator=g) < 0.5), torch.tensor(JUNK[dt], dtype=DTYPES[dt]), dst)
    return src, dst


@lru_cache(maxsize=None)
def expected(B: int, H: int, W: int, dt: str, ramp, seed: int = 17) -> torch.Tensor:
    """the reference of `pair`, computed once"""
    return paste_expected(*pair(B, H, W, dt, ramp, seed), ramp, dt)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    return bool(image_exact.same_bits(got, want).all())
