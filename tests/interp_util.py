"""Shapes, inputs and the float64 checker of the plain-interpolation tests (mz_interpolate, ultrazoom_amd/interpolate.py); shared by
tests/test_interp_cpu.py, tests/test_interp_gpu.py and tests/test_poison_interp_gpu.py.  The gates are those of the resampling tests
(resize_util.assert_within_gate; tests/test_resize_gpu.py has their reasons)."""

import re
from functools import lru_cache
from pathlib import Path

import torch
import torch.nn.functional as F

from degrade_ref import as_double
from resize_util import DTYPES, ELEM, assert_within_gate, image, shape_id  # noqa: F401  (re-exported to the interpolation tests)

HEADER = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_interp.h").read_text()
TILE_H = int(re.search(r"constexpr int kInterpTileH = (\d+);", HEADER).group(1))
TILE_W = int(re.search(r"constexpr int kInterpTileW = (\d+);", HEADER).group(1))
STAGE_ROWS = int(re.search(r"constexpr int kInterpStageRows = (\d+);", HEADER).group(1))
MODES = ("nearest", "bilinear", "bicubic")
MODE = {"nearest": 0, "bilinear": 1, "bicubic": 2}

# three tile rows and columns with ragged last ones: enlarged by about two (the separable path) and halved (the gather path)
RAGGED_OUT = (2 * TILE_H + 1, 3 * TILE_W - 1)
RAGGED_UP = (((RAGGED_OUT[0] + 1) // 2, (RAGGED_OUT[1] + 1) // 2), RAGGED_OUT)
RAGGED_DOWN = ((2 * RAGGED_OUT[0], 2 * RAGGED_OUT[1]), RAGGED_OUT)
UP3 = ((24, 40), (72, 120))
SHAPES = [((9, 11), (18, 22)), ((9, 11), (36, 44)), ((9, 11), (72, 88)), ((7, 5), (10, 13)), ((33, 35), (8, 9)), ((1, 1), (5, 7)),
          ((5, 7), (1, 1)), UP3, RAGGED_UP, RAGGED_DOWN]


def want64_of(x: torch.Tensor, size, mode: str) -> torch.Tensor:
    """torch's own interpolate without antialiasing, in float64 on the CPU (bilinear, bicubic)"""
    return F.interpolate(as_double(x), size=tuple(size), mode=mode, align_corners=False)


def nearest_index(n_in: int, n_out: int) -> torch.Tensor:
    """The source index of every output index of one axis as torch's legacy "nearest" picks it (float32 arithmetic): its float32 CPU
    kernel applied to the indices themselves, which are exact in float32 below 2^24"""
    assert n_in < (1 << 24)
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(ramp, size=(n_out, 1), mode="nearest").flatten().long()


def nearest_of(x: torch.Tensor, size) -> torch.Tensor:
    """torch's legacy nearest as a pure gather (every element type, bit patterns untouched)"""
    x = x.cpu()
    return x[:, :, nearest_index(x.shape[2], size[0])][:, :, :, nearest_index(x.shape[3], size[1])]


def bits(t: torch.Tensor) -> torch.Tensor:
    """the elements as integers: equality of bit patterns, NaN payloads and -0 included"""
    t = t.cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


NOISE_FLOOR = 1e-12


@lru_cache(maxsize=None)
def gate_seed(B: int, shape, dt: str) -> int:
    """The seed of the input that a case's gate is applied to, found from the CHECKER alone: the first one from 7 upwards whose float64
    results all have a magnitude of at least 1e-12.  The gate of the 16-bit types is relative -- one ulp of the storage type AT the
    float64 value -- and means nothing where that value is the checker's own rounding noise: rounded to bfloat16, neighbouring
    pixels are often in a simple ratio, and e.g. 10 / 9 a - 1 / 9 (10 a), a x3 bicubic at the top edge, is exactly 0, of which torch's float64
    kernel leaves -6.8e-17 and a sum in another order -1.1e-16: "96 ulps" apart (seed 7 of the 3 x 24 x 40 bf16 image holds that pair)."""
    if dt == "u8":
        return 7  # (an absolute gate)
    for seed in range(7, 39):
        x = image(B, *shape[0], dt, seed)
        if all(float(want64_of(x, shape[1], mode).abs().min()) >= NOISE_FLOOR for mode in ("bilinear", "bicubic")):
            return seed
    raise AssertionError(f"no usable input for {B} x {shape} {dt}")


def gate_image(B: int, shape, dt: str) -> torch.Tensor:
    return image(B, *shape[0], dt, gate_seed(B, shape, dt))


@lru_cache(maxsize=None)
def checker(B: int, shape, dt: str, mode: str) -> torch.Tensor:
    """The checker of gate_image(B, shape, dt), once per case; left unchanged by its users"""
    return want64_of(gate_image(B, shape, dt), shape[1], mode)


def hip_interp(x, size=None, scale_factor=None, **kw):
    from ultrazoom_amd.interpolate import interpolate

    return interpolate(x, size, scale_factor, **kw)
