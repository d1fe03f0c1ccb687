"""mz_yuv420_to_rgb and mz_rgb_to_yuv420 in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_color_gpu.py:
the inputs between NaN guards (0xFF bytes; uint8 data also between 0x00 guards), the outputs between pattern guards, dense and strided.
The results have the bits of the reference -- so no poisoned byte next to an input has reached an output -- and no guard and no input
has changed.  A test of loads and stores staying inside their tensors: every run here is an ordinary, valid call."""

import pytest
import torch

import color_ref
import yuv_ref
from color_ref import DTYPES, ELEM
from poison_util import Arena
from ultrazoom_amd import _ffi
from yuv_ref import MATRIX_CODE, RANGE_CODE, SITING_CODE

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 3), (2, 17), (4, 32), (5, 33), (7, 129)]
B = 2
CASES = [("bt709", "limited", "left"), ("bt601", "full", "center")]


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def codes(matrix, range_, siting):
    return MATRIX_CODE[matrix], RANGE_CODE[range_], SITING_CODE[siting]


def same_planes(got, want):
    return all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("guard", [0xFF, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_yuv420_to_rgb_touches_its_tensors_only(shape, dt, guard):
    H, W = shape
    hc, wc = yuv_ref.chroma_hw(H, W)
    y, cb, cr = yuv_ref.planes(B, H, W)
    for case in CASES:
        want = color_ref.store(yuv_ref.rgb_f64(B, H, W, *case), dt, 1)
        # dense planes, a dense result: the wide accesses wherever a row holds a whole run
        arena = Arena("cuda")
        ya, cba, cra = (arena.input(t.cuda(), name=n, fill=guard) for t, n in ((y, "y"), (cb, "cb"), (cr, "cr")))
        out = arena.output((B, 3, H, W), DTYPES[dt], fill=3, name="out")
        _ffi.yuv420_to_rgb(_ffi.pair(ya), _ffi.pair(cba), _ffi.pair(cra), _ffi.pair(out), ELEM[dt], B, H, W, *codes(*case), 1, stream())
        arena.check()
        assert color_ref.same_bits(out, want), case
        # interleaved chroma pairs in (one input, the two views one byte apart), an interleaved HWC frame out
        arena = Arena("cuda")
        ya = arena.input(y.cuda(), name="y", fill=guard)
        pairs = arena.input(torch.stack([cb, cr], dim=-1).cuda(), name="pairs", fill=guard)
        out = arena.output((B, H, W, 3), DTYPES[dt], fill=3, name="out_hwc").permute(0, 3, 1, 2)
        _ffi.yuv420_to_rgb(_ffi.pair(ya), _ffi.pair(pairs[..., 0]), _ffi.pair(pairs[..., 1]), _ffi.pair(out), ELEM[dt], B, H, W, *codes(*case), 1, stream())
        arena.check()
        assert color_ref.same_bits(out.contiguous(), want), case
        assert tuple(pairs[..., 0].shape) == (B, 1, hc, wc)


@pytest.mark.parametrize("guard", [0xFF, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_to_yuv420_touches_its_tensors_only(shape, dt, guard):
    H, W = shape
    hc, wc = yuv_ref.chroma_hw(H, W)
    x = color_ref.image(B, H, W, dt).cuda()
    for case in CASES:
        want = yuv_ref.yuv_of_image(B, H, W, dt, *case)
        # a dense image in, dense planes out
        arena = Arena("cuda")
        xa = arena.input(x, name="x", fill=guard)
        ya = arena.output((B, 1, H, W), torch.uint8, fill=3, name="y")
        cba, cra = (arena.output((B, 1, hc, wc), torch.uint8, fill=3, name=n) for n in ("cb", "cr"))
        _ffi.rgb_to_yuv420(_ffi.pair(xa), ELEM[dt], _ffi.pair(ya), _ffi.pair(cba), _ffi.pair(cra), B, H, W, *codes(*case), stream())
        arena.check()
        assert same_planes((ya, cba, cra), want), case
        # an interleaved HWC frame in; Cb with a column stride of 2 into one buffer, Cr dense into another: the odd bytes of the first
        # buffer keep what they held
        arena = Arena("cuda")
        xa = arena.input(x.permute(0, 2, 3, 1), name="x_hwc", fill=guard).permute(0, 3, 1, 2)
        ya = arena.output((B, 1, H, 2 * W), torch.uint8, fill=3, name="y_wide")
        cbw = arena.output((B, 1, hc, 2 * wc), torch.uint8, fill=3, name="cb_wide")
        cra = arena.output((B, 1, hc, wc), torch.uint8, fill=3, name="cr")
        _ffi.rgb_to_yuv420(_ffi.pair(xa), ELEM[dt], _ffi.pair(ya[..., ::2]), _ffi.pair(cbw[..., ::2]), _ffi.pair(cra), B, H, W, *codes(*case),
                           stream())
        arena.check()
        assert same_planes((ya[..., ::2], cbw[..., ::2], cra), want), case
        assert bool((cbw[..., 1::2] == 3).all()) and bool((ya[..., 1::2] == 3).all())
        # interleaved pairs out (one output, the two views one byte apart), Cr first: both planes in one 16-byte store where a run is whole
        arena = Arena("cuda")
        xa = arena.input(x, name="x", fill=guard)
        ya = arena.output((B, 1, H, W), torch.uint8, fill=3, name="y")
        pairs = arena.output((B, 1, hc, wc, 2), torch.uint8, fill=3, name="pairs")
        _ffi.rgb_to_yuv420(_ffi.pair(xa), ELEM[dt], _ffi.pair(ya), _ffi.pair(pairs[..., 1]), _ffi.pair(pairs[..., 0]), B, H, W, *codes(*case), stream())
        arena.check()
        assert same_planes((ya, pairs[..., 1], pairs[..., 0]), want), case
