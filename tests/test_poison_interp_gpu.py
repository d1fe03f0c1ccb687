"""mz_interpolate in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_resize_gpu.py: the input between NaN
guards (uint8: 0xFF and 0x00 guards), the output between pattern guards, dense and strided, whole and windowed, every mode and element
type.  The result has the bits of the run on ordinary tensors, no guard and no input has changed.  A test of loads and stores staying
inside their tensors: every run here is an ordinary, valid call."""

import pytest
import torch

from interp_util import DTYPES, ELEM, MODE, RAGGED_DOWN, RAGGED_UP, UP3, hip_interp, image, shape_id
from poison_util import Arena
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

CASES = [(UP3, None), (RAGGED_UP, None), (RAGGED_DOWN, None), (RAGGED_UP, (5, 29, 40, 300)), (RAGGED_DOWN, (33, 255, 32, 128)),
         (UP3, (70, 100, 2, 20)), (((5, 7), (1, 1)), None), (((1, 1), (5, 7)), None)]
POISONS = [(dt, 0xFF) for dt in sorted(DTYPES)] + [("u8", 0x00)]  # 0xFF bytes are NaN in the floating-point types; uint8 gets both


def case_id(c):
    return shape_id(c[0]) + ("" if c[1] is None else "_window")


@pytest.mark.parametrize("mode", sorted(MODE))
@pytest.mark.parametrize("dt, guard", POISONS, ids=[f"{d}_{g:02x}" for d, g in POISONS])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_interpolate_touches_its_tensors_only(case, dt, guard, mode):
    ((hin, win), size), window = case
    B = 2
    x = image(B, hin, win, dt).cuda()
    want = hip_interp(x, size, mode=mode, window=window)
    stream = torch.cuda.current_stream().cuda_stream
    # dense views
    arena = Arena("cuda")
    xa = arena.input(x, name="x", fill=guard)
    out = arena.output(tuple(want.shape), DTYPES[dt], fill=3, name="out")
    _ffi.interpolate(xa.data_ptr(), xa.stride(), out.data_ptr(), out.stride(), ELEM[dt], B, hin, win, size[0], size[1], MODE[mode], 0, window,
                     stream)
    arena.check()
    if dt != "u8":
        assert not bool(torch.isnan(out).any())
    assert torch.equal(out, want)
    # strided views: an interleaved HWC frame in, one out (the element path on both sides)
    arena = Arena("cuda")
    xa = arena.input(x.permute(0, 2, 3, 1), name="x_hwc", fill=guard).permute(0, 3, 1, 2)
    h, w = want.shape[-2:]
    out = arena.output((B, h, w, 3), DTYPES[dt], fill=3, name="out_hwc").permute(0, 3, 1, 2)
    _ffi.interpolate(xa.data_ptr(), xa.stride(), out.data_ptr(), out.stride(), ELEM[dt], B, hin, win, size[0], size[1], MODE[mode], 0, window,
                     stream)
    arena.check()
    assert torch.equal(out, want)
