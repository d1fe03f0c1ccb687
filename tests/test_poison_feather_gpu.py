"""mz_feather_paste in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_alpha_gpu.py: src between 0xFF
(NaN) or 0x00 guards, dst between pattern guards and pre-filled with NaN bytes (0xFF) under every element with w == 1, where the paste
moves src and must not look at dst.  The result has the bits of the reference -- so no poisoned byte next to an input and no byte dst
held under w == 1 has reached it -- and no guard and no byte of src has changed.  A test of loads and stores staying inside their
tensors: every run here is an ordinary, valid call."""

import numpy as np
import pytest
import torch

import feather_ref
from feather_ref import DTYPES, ELEM, same_bits
from poison_util import Arena
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(1, 1), (5, 3), (9, 8), (17, 33), (6, 34)]  # one element; less than a run; whole runs of float32; ragged runs behind whole ones
RAMPS = [(0, 0), (2, 3), (0, 4), (6, 10), (3, 0)]


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def poisoned_dst(dst: torch.Tensor, H: int, W: int, ramp) -> torch.Tensor:
    """dst with every bit set under w == 1"""
    w1 = torch.from_numpy(np.broadcast_to(feather_ref.weights(H, W, *ramp) == 1.0, dst.shape).copy())
    out = dst.clone()
    feather_ref.bits(out)[w1] = -1 if dst.element_size() > 1 else 0xFF
    return out


def _paste_touches_its_tensors_only(layout, dt):
    for (H, W), ramp in zip(SHAPES, RAMPS):
        src, dst = feather_ref.pair(B, H, W, dt, ramp)
        dst = poisoned_dst(dst, H, W, ramp)
        want = feather_ref.paste_expected(src, dst, ramp, dt)
        for guard in (0xFF, 0x00):
            arena = Arena("cuda")
            if layout == "planar":
                s = arena.input(src.cuda(), name="src", fill=guard)
                d = arena.output((B, 3, H, W), DTYPES[dt], fill=3, name="dst")
            else:
                s = arena.input(src.permute(0, 2, 3, 1).contiguous().cuda(), name="src", fill=guard).permute(0, 3, 1, 2)
                full = arena.output((B, H, W, 4), DTYPES[dt], fill=3, name="dst").permute(0, 3, 1, 2)
                d = full[:, :3]
            d.copy_(dst)
            _ffi.feather_paste(_ffi.pair(s), _ffi.pair(d), ELEM[dt], B, H, W, ramp[0], ramp[1], stream())
            arena.check()
            assert same_bits(d.contiguous(), want), (H, W, ramp, guard)
            if layout == "hwc":  # the fourth element of every pixel of dst keeps its fill
                assert bool((full[:, 3] == 3).all())


@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_paste_touches_its_tensors_only(layout):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _paste_touches_its_tensors_only(layout, dt)
