"""mz_resize in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_ops_gpu.py: the input between NaN guards
(uint8: 0xFF and 0x00 guards), the output between pattern guards, the workspace pre-filled with 0xFF bytes (NaN as float64, -1 as a tap
count) between pattern guards.  The result has the bits of the run on ordinary tensors, no guard and no input has changed.  A test of
loads and stores staying inside their tensors: every run here is an ordinary, valid call."""

import pytest
import torch

from poison_util import Arena
from resize_util import DTYPES, ELEM, RAGGED, TAPS66, UP3, hip_resize, image, shape_id
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

CASES = [(TAPS66, None), (UP3, None), (RAGGED, None), (RAGGED, (5, 29, 10, 40)), (UP3, (70, 100, 2, 20))]
POISONS = [(dt, 0xFF) for dt in sorted(DTYPES)] + [("u8", 0x00)]  # 0xFF bytes are NaN in the floating-point types; uint8 gets both


def case_id(c):
    return shape_id(c[0]) + ("" if c[1] is None else "_window")


@pytest.mark.parametrize("filt", [0, 1], ids=["bicubic", "bilinear"])
@pytest.mark.parametrize("dt, guard", POISONS, ids=[f"{d}_{g:02x}" for d, g in POISONS])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_resize_touches_its_tensors_only(case, dt, guard, filt):
    ((hin, win), size), window = case
    B = 2
    x = image(B, hin, win, dt).cuda()
    want = hip_resize(x, size, filter=("bicubic", "bilinear")[filt], window=window)
    arena = Arena("cuda")
    xa = arena.input(x, name="x", fill=guard)
    out = arena.output(tuple(want.shape), DTYPES[dt], fill=3, name="out")
    need = _ffi.resize_workspace_bytes(hin, win, size[0], size[1], filt)
    ws = arena.raw(need, 0xFF, name="workspace")
    _ffi.resize(xa.data_ptr(), xa.stride(), out.data_ptr(), out.stride(), ELEM[dt], B, hin, win, size[0], size[1], filt, 0, window,
                ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    arena.check()
    if dt != "u8":
        assert not bool(torch.isnan(out).any())
    assert torch.equal(out, want)
