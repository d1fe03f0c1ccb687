"""Shapes, inputs, the float64 checker and the gates of the resampling tests (tests/test_resize_gpu.py has the gates' reasons); shared
with tests/test_resize_cpu.py, tests/test_poison_resize_gpu.py and the blur tests of tests/test_degrade_gpu.py."""

import re
from functools import lru_cache
from pathlib import Path

import torch
import torch.nn.functional as F

from degrade_ref import as_double
from golden_util import GoldenCase
from gpu_util import ulp_of
from ultrazoom_amd import MewZoom

HEADER = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_resize.h").read_text()
TILE_H = int(re.search(r"constexpr int kResizeTileH = (\d+);", HEADER).group(1))
TILE_W = int(re.search(r"constexpr int kResizeTileW = (\d+);", HEADER).group(1))
RAGGED = ((2 * (2 * TILE_H + 1), 2 * (3 * TILE_W - 1)), (2 * TILE_H + 1, 3 * TILE_W - 1))  # three tile rows and columns, ragged last ones
UP3 = ((24, 40), (72, 120))
TAPS66 = ((160, 40), (10, 40))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.uint8}
ELEM = {"f32": 0, "bf16": 1, "f16": 2, "u8": 3}
FILTERS = ("bicubic", "bilinear")


def shape_id(s):
    return f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}"


@lru_cache(maxsize=None)
def image(B: int, H: int, W: int, dt: str, seed: int = 7) -> torch.Tensor:
    """uniform noise in [0, 1], rounded to the element type, on the CPU"""
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed + 1000 * B + H * W), dtype=torch.float32)
    return (x * 255.0).round().to(torch.uint8) if dt == "u8" else x.to(DTYPES[dt])


def want64_of(x: torch.Tensor, size, filt: str) -> torch.Tensor:
    """torch's float64 antialiased interpolate.  Its CPU kernel gives an output of ONE column and several rows wrong (5 x 1 -> 2 x 1: both
    rows come out equal; it disagrees with its own weight matrices and with its own result for the transposed image, by 0.2 - 0.4 on
    [0, 1] data), so such a size runs transposed: the filter is separable and the same on both axes, the function and the float64
    arithmetic are the same.  tests/test_resize_cpu.py holds this checker to torch's weight matrices at those sizes."""
    xd = as_double(x)
    if size[1] == 1 and size[0] > 1:
        return F.interpolate(xd.transpose(-1, -2).contiguous(), size=(1, size[0]), mode=filt, antialias=True, align_corners=False).transpose(-1, -2)
    return F.interpolate(xd, size=tuple(size), mode=filt, antialias=True, align_corners=False)


def hip_resize(x, size, **kw):
    from ultrazoom_amd.resize import resize

    return resize(x, size, **kw)


def assert_within_gate(got: torch.Tensor, want64: torch.Tensor, dt: str, what: str) -> None:
    got = got.cpu()
    assert got.dtype == DTYPES[dt] and got.shape == want64.shape, (what, got.dtype, got.shape)
    if dt == "u8":
        scaled = want64.clamp(0, 1) * 255
        want = torch.floor(scaled + 0.5)
        near_tie = ((scaled - torch.floor(scaled)) - 0.5).abs() <= 1e-3
        diff = (got.double() - want).abs()
        exact_tie = ((scaled - torch.floor(scaled)) - 0.5).abs() <= 1e-9
        share = float((near_tie & ~exact_tie).double().mean())
        print(f"{what}: {int((diff != 0).sum())} of {diff.numel()} elements differ, {share:.4%} lie within 1e-3 of a tie, "
              f"{float(exact_tie.double().mean()):.4%} on one")
        assert share < 0.01, (what, share)
        assert bool((diff[~near_tie] == 0).all()), (what, int((diff[~near_tie] != 0).sum()))
        assert float(diff.max()) <= 1, (what, float(diff.max()))
        return
    diff = (got.double() - want64).abs()
    print(f"{what}: max-abs {float(diff.max()):.3e}")
    if dt == "f32":
        assert float(diff.max()) <= 1e-5, (what, float(diff.max()))
    else:
        excess = diff / ulp_of(want64, dt).double()
        assert float(excess.max()) <= 1.0, (what, float(excess.max()), float(diff.max()))


@lru_cache(maxsize=None)
def model_and_input(dt: str):
    case = GoldenCase("g3_4x_c16")
    assert (case.B, case.H, case.W) == (1, 24, 40) and case.config["upscale_ratio"] == 4, (case.B, case.H, case.W, case.config)
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    return m.to("cuda", DTYPES[dt]).eval(), case.image().to("cuda", DTYPES[dt])
