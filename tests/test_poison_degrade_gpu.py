"""mz_blur, mz_noise and mz_jpeg in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_resize_gpu.py: the
input between NaN guards (uint8: 0xFF and 0x00 guards), the output between pattern guards, the JPEG workspace pre-filled with 0xFF bytes
between pattern guards.  The result has the bits of the run on ordinary tensors, no guard and no input has changed.  A test of loads
and stores staying inside their tensors: every run here is an ordinary, valid call."""

import pytest
import torch

from degrade_ref import DTYPES, ELEM, hip, image, shape_id
from poison_util import Arena
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

SHAPES = [(17, 33), (37, 45)]
POISONS = [(dt, 0xFF) for dt in sorted(DTYPES)] + [("u8", 0x00)]  # 0xFF bytes are NaN in the floating-point types; uint8 gets both
B = 2


@pytest.mark.parametrize("dt, guard", POISONS, ids=[f"{d}_{g:02x}" for d, g in POISONS])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_the_degradation_entries_touch_their_tensors_only(shape, dt, guard):
    H, W = shape
    x = image(B, H, W, dt).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    want = {"blur": hip().gaussian_blur(x, 2.5), "noise": hip().gaussian_noise(x, 0.1, seed=9, offset=2), "jpeg": hip().jpeg(x, 50)}
    arena = Arena("cuda")
    xa = arena.input(x, name="x", fill=guard)
    outs = {k: arena.output(tuple(x.shape), DTYPES[dt], fill=3, name=k) for k in want}
    need = _ffi.jpeg_workspace_bytes(B, H, W)
    ws = arena.raw(need, 0xFF, name="workspace")
    _ffi.blur(xa.data_ptr(), xa.stride(), outs["blur"].data_ptr(), outs["blur"].stride(), ELEM[dt], B, H, W, 2.5, stream)
    _ffi.noise(xa.data_ptr(), xa.stride(), outs["noise"].data_ptr(), outs["noise"].stride(), ELEM[dt], B, H, W, 0.1, 9, 2, stream)
    _ffi.jpeg(xa.data_ptr(), xa.stride(), outs["jpeg"].data_ptr(), outs["jpeg"].stride(), ELEM[dt], B, H, W, 50, ws.data_ptr(), need, stream)
    arena.check()
    for k, out in outs.items():
        if dt != "u8":
            assert not bool(torch.isnan(out).any()), k
        assert torch.equal(out, want[k]), k
    # in place, the one entry that allows it: the input's guards still hold, its contents are the result
    inplace = Arena("cuda")
    y = inplace.output(tuple(x.shape), DTYPES[dt], fill=3, name="in place")
    y.copy_(x)
    _ffi.noise(y.data_ptr(), y.stride(), y.data_ptr(), y.stride(), ELEM[dt], B, H, W, 0.1, 9, 2, stream)
    inplace.check()
    assert torch.equal(y, want["noise"])
