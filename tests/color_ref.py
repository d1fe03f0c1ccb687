"""Exact-arithmetic reference of the luma entries (tests/test_color_cpu.py, tests/test_color_gpu.py, tests/test_poison_color_gpu.py):
ultrazoom_amd/csrc/mz_color.h restated in Python from the header alone -- nothing here calls the library.  Needs no GPU.

  COEFFS           {off, kr, kg, kb} of each standard: Python-float divisions, as the header writes them
  luma_f64         the unrounded float64 Y plane: acc = off, then acc = fma(k, v, acc) for R, G, B (image_exact.fma64); a uint8 element
                   v is v / 255.0 by true division
  store            the one rounding to the stored type, per dtype
  luma_expected    the tensor mz_luma stores
  u8_ties          the uint8 colours whose Y * 255 is EXACTLY k + 1/2 in rational arithmetic, the only colours at which the float64
                   arithmetic's own roundings decide the byte
  SHAPES, image    the cases of the GPU test and their inputs, every one chosen from the reference alone

What the search of u8_ties finds over the 2^24 colours (tests/test_color_cpu.py asserts these counts).  Y * 255 is, exactly,
16 + (65481 r + 128553 g + 24966 b) / 255000 for "bt601" and (299 r + 587 g + 114 b) / 1000 for "full"; every other colour is at least
1 / 255000 from a tie, nine orders above the float64 error.  "bt601": 194 exact ties, of which the float64 arithmetic puts 142 on
k + 1/2 exactly (stored k + 1), 43 a few units in the last place below it (stored k) and 9 above; "full": 16 782 exact ties, 11 052 on
k + 1/2, 4 850 below, 880 above (TIE_CENSUS).  The planted pixels of `image` are taken from both lists, twelve of each, evenly spaced.

fp16: NO finite input makes Y overflow -- the weights of either standard are positive and add up to at most 1 (0.8588 for "bt601"), so Y
of the largest finite value, 65504, is at most 65504 < 65520, the overflow tie.  The nearest there is is planted instead: pixels of
+-65504 (Y rounds to +-65504 in "full"), and an infinity pixel, whose Y is the infinity itself."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

import image_exact
from image_exact import F32, F64, fma64

COEFFS = {"bt601": (16.0 / 255.0, 65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0), "full": (0.0, 0.299, 0.587, 0.114)}
CODE = {"bt601": 0, "full": 1}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.uint8}
ELEM = {"f32": 0, "bf16": 1, "f16": 2, "u8": 3}
# (H, W): one pixel; a row below, at and above one 16-byte run of uint8; two rows whose ends are partial runs; several workgroups' worth of
# runs in float32 (7 x 129: 231 runs a plane)
SHAPES = [(1, 1), (1, 15), (1, 16), (1, 17), (3, 31), (2, 33), (5, 64), (7, 129)]


def values(x: torch.Tensor) -> np.ndarray:
    """the float64 value of every element: ld_f64 of mz_view.h"""
    x = x.cpu()
    return x.numpy().astype(F64) / 255.0 if x.dtype == torch.uint8 else x.double().numpy()


def luma_f64(x: torch.Tensor, standard: str) -> np.ndarray:
    """[B, 3, H, W] of any of the four dtypes -> the unrounded Y, float64 [B, 1, H, W]"""
    off, kr, kg, kb = COEFFS[standard]
    v = values(x)
    acc = np.full(v[:, 0:1].shape, off, dtype=F64)
    acc = fma64(kr, v[:, 0:1], acc)
    acc = fma64(kg, v[:, 1:2], acc)
    return fma64(kb, v[:, 2:3], acc)


def store(y: np.ndarray, dt: str, clamp: int) -> torch.Tensor:
    """luma_round_raw of mz_color.h.  The clamp is fmin(fmax(v, 0), 1): a NaN becomes 0.
    f32: the cast; bf16, f16: ONE rounding of the float64 value to nearest even; u8: always the clamp, then * 255 and + 0.5 as two
    float64 operations, then truncation."""
    with np.errstate(all="ignore"):
        if dt == "u8":
            t = image_exact.clamp01(y) * 255.0
            return torch.from_numpy((t + 0.5).astype(np.uint8))
        if clamp:
            y = image_exact.clamp01(y)
        if dt == "f32":
            return torch.from_numpy(y.astype(F32))
        return image_exact.round64(y, dt)


def luma_expected(x: torch.Tensor, standard: str, dt: str, clamp: int) -> torch.Tensor:
    assert x.dtype == DTYPES[dt], (x.dtype, dt)
    return store(luma_f64(x, standard), dt, clamp)


# ---- uint8 rounding ties ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def u8_ties(standard: str) -> np.ndarray:
    """[n, 3] uint8: the colours (r, g, b) whose exact Y * 255 is k + 1/2, in ascending order of (r, g, b)"""
    (wr, wg, wb), den = ((65481, 128553, 24966), 255000) if standard == "bt601" else ((299, 587, 114), 1000)
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    gb = wg * g + wb * b
    found = []
    for r in range(256):
        gi, bi = np.nonzero((wr * r + gb) % den == den // 2)
        found += [(r, int(a), int(c)) for a, c in zip(gi, bi)]
    return np.array(found, dtype=np.uint8).reshape(-1, 3)


TIE_CENSUS = {"bt601": (194, 142, 43, 9), "full": (16782, 11052, 4850, 880)}  # what tie_census finds (tests/test_color_cpu.py)


def tie_census(standard: str):
    """(exact ties, those whose float64 clamp(Y) * 255 is k + 1/2 exactly, those below it, those above it)"""
    c = u8_ties(standard)
    x = torch.from_numpy(c.T.reshape(1, 3, 1, -1).copy())
    t = image_exact.clamp01(luma_f64(x, standard)) * 255.0
    frac = t - np.floor(t)
    return len(c), int((frac == 0.5).sum()), int((frac < 0.5).sum()), int((frac > 0.5).sum())


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
TINY = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}  # the smallest subnormal of the type
HUGE = {"f32": float(np.finfo(F32).max), "bf16": float(torch.finfo(torch.bfloat16).max), "f16": 65504.0}


def special_pixels(dt: str):
    """(r, g, b) triples planted at the first pixels of image 0 (as many as the image has room for)"""
    if dt == "u8":
        px = [(255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)]
        for standard in ("bt601", "full"):
            c = u8_ties(standard)
            px += [tuple(int(v) for v in c[i]) for i in np.linspace(0, len(c) - 1, 12).astype(int)]
        return px
    inf, nan, tiny, huge = float("inf"), float("nan"), TINY[dt], HUGE[dt]
    return [(-0.0, -0.0, -0.0), (tiny, tiny, tiny), (-tiny, 3 * tiny, -tiny), (1.0, 1.0, 1.0), (inf, 0.5, 0.25), (0.5, nan, 0.25),
            (huge, huge, huge), (-huge, -huge, -huge), (0.25, -inf, 0.5), (inf, -inf, 0.0), (0.0, 0.0, 0.0), (-0.75, 2.5, 1.5),
            (2.0 ** -126 * 0.75, 0.0, -0.0)]


@lru_cache(maxsize=None)
def image(B: int, H: int, W: int, dt: str, seed: int = 5, special: bool = True) -> torch.Tensor:
    """[B, 3, H, W] on the CPU, built once and left unchanged by its users: noise over [-0.25, 1.25] rounded to the type (uint8: all
    bytes), the special pixels in front of image 0"""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    if dt == "u8":
        x = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    else:
        x = (torch.rand((B, 3, H, W), generator=g, dtype=torch.float64) * 1.5 - 0.25).to(DTYPES[dt])
    if special:
        flat = x[0].reshape(3, H * W)
        for i, px in enumerate(special_pixels(dt)[: H * W]):
            flat[:, i] = torch.tensor(px, dtype=torch.float64).to(DTYPES[dt])
    return x


@lru_cache(maxsize=None)
def expected(B: int, H: int, W: int, dt: str, standard: str, clamp: int) -> torch.Tensor:
    """the reference of `image`, computed once"""
    return luma_expected(image(B, H, W, dt), standard, dt, clamp)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    return bool(image_exact.same_bits(got, want).all())


# ---- the luma plan (mz_metrics.h, metrics_plan with C = 1) ---------------------------------------------------------------------------------
TILE_H, TILE_W, PSNR_BLOCKS_MAX = 16, 32, 512


def metrics_plan_bytes(B: int, H: int, W: int, which: int, C: int = 3, luma: bool = False) -> int:
    """the workspace of mz_metrics (C = 3) and of mz_metrics_luma (C = 1, luma: the two float64 Y planes behind it)"""
    total = 0

    def take(n):
        nonlocal total
        total += (n + 255) // 256 * 256

    def tiles(h, w, taps):
        return -(-(h - taps + 1) // TILE_H) * -(-(w - taps + 1) // TILE_W)

    planes = B * C
    take(B * min(C * H, PSNR_BLOCKS_MAX) * 5 * 8)
    take(8)
    if which & 2:
        take(planes * tiles(H, W, 11) * 8)
    if which & 4:
        h, w = H, W
        for s in range(4):
            n = 2 ** (4 - s) + 1
            if s:
                h, w = (h - n + 2) // 2, (w - n + 2) // 2
                take(2 * planes * h * w * 8)
            take(planes * tiles(h, w, n) * 2 * 8)
    if luma:
        take(2 * B * H * W * 8)
    return total
