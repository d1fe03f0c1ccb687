"""mz_alpha_fill and mz_alpha_merge in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_ycbcr_gpu.py: the
inputs between 0xFF (NaN) or 0x00 guards, the outputs between pattern guards, the workspace of EXACTLY the stated bytes between pattern
guards and pre-filled with NaN bytes or zeros.  The results have the bits of the reference -- so no poisoned byte next to an input and no
byte the workspace held has reached an output -- and no guard and no input has changed.  A test of loads and stores staying inside their
tensors: every run here is an ordinary, valid call."""

import pytest
import torch

import alpha_ref
from alpha_ref import DTYPES, ELEM, same_bits
from poison_util import Arena
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(1, 1), (5, 3), (9, 8), (17, 33), (4, 32), (6, 34)]  # one pixel; odd levels; whole 16-byte runs; a ragged run behind whole ones


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _fill_touches_its_tensors_and_its_workspace_only(layout, dt):
    for (H, W), premultiplied in zip(SHAPES, (0, 1) * 3):
        x = alpha_ref.rgba(B, H, W, dt)
        if premultiplied:
            x = alpha_ref.premultiplied_of(x, dt)
        want = alpha_ref.fill_expected(x[:, :3], x[:, 3:4], dt, bool(premultiplied))
        need = _ffi.alpha_fill_workspace_bytes(B, H, W)
        assert need == alpha_ref.workspace_bytes(B, H, W)
        for guard, ws_fill in ((0xFF, 0xFF), (0x00, 0x00), (0xFF, 0x00)):
            arena = Arena("cuda")
            if layout == "planar":
                xa = arena.input(x.cuda(), name="x", fill=guard)
                out = arena.output((B, 3, H, W), DTYPES[dt], fill=3, name="out")
            else:
                xa = arena.input(x.permute(0, 2, 3, 1).contiguous().cuda(), name="x", fill=guard).permute(0, 3, 1, 2)
                full = arena.output((B, H, W, 4), DTYPES[dt], fill=3, name="out").permute(0, 3, 1, 2)
                out = full[:, :3]
            ws = arena.raw(need, ws_fill, name="workspace")
            _ffi.alpha_fill(_ffi.pair(xa[:, :3]), _ffi.pair(xa[:, 3:4]), _ffi.pair(out), ELEM[dt], B, H, W, premultiplied, ws.data_ptr(), need, stream())
            arena.check()
            assert same_bits(out.contiguous(), want), (H, W, premultiplied, guard, ws_fill)
            if layout == "hwc":  # the fourth element of every output pixel keeps its fill
                assert bool((full[:, 3] == 3).all())


@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_fill_touches_its_tensors_and_its_workspace_only(layout):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _fill_touches_its_tensors_and_its_workspace_only(layout, dt)


def _merge_touches_its_tensors_only(layout, dt):
    for ((H, W), size), mode, premultiply in zip((((5, 3), (10, 6)), ((9, 11), (20, 31)), ((4, 8), (32, 64)), ((9, 8), (9, 8))),
                                                 ("bicubic", "bilinear", "bicubic", "nearest"), (1, 0, 1, 1)):
        x = alpha_ref.rgba(B, H, W, dt)
        sr = alpha_ref.rgba(B, size[0], size[1], dt, seed=23)[:, :3].contiguous()
        want_alpha, want_rgb = alpha_ref.merge_expected(sr, x[:, 3:4], size, mode, dt, bool(premultiply))
        for guard in (0xFF, 0x00):
            arena = Arena("cuda")
            alpha = arena.input(x[:, 3:4].contiguous().cuda(), name="alpha", fill=guard)
            sra = arena.input(sr.cuda(), name="sr", fill=guard)
            if layout == "planar":
                out = arena.output((B, 4) + size, DTYPES[dt], fill=3, name="out")
            else:
                out = arena.output((B,) + size + (4,), DTYPES[dt], fill=3, name="out").permute(0, 3, 1, 2)
            pairs = (_ffi.pair(sra), _ffi.pair(out[:, :3])) if premultiply else (None, None)
            _ffi.alpha_merge(pairs[0], _ffi.pair(alpha), pairs[1], _ffi.pair(out[:, 3:4]), ELEM[dt], B, H, W, size[0], size[1], alpha_ref.MODES[mode],
                             premultiply, stream())
            arena.check()
            assert same_bits(out[:, 3:4].contiguous(), want_alpha), (H, W, mode, guard)
            if premultiply:
                assert same_bits(out[:, :3].contiguous(), want_rgb), (H, W, mode, guard)
            else:
                assert bool((out[:, :3] == 3).all())


@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_merge_touches_its_tensors_only(layout):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _merge_touches_its_tensors_only(layout, dt)
