"""mz_luma and mz_metrics_luma in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_interp_gpu.py: the
inputs between NaN guards (uint8: 0xFF and 0x00 guards), the outputs and the workspace between pattern guards, dense and strided.  The
results have the bits of the run on ordinary tensors, no guard and no input has changed, and whatever the workspace held on entry -- NaN
bytes or a pattern -- the metrics have the same bits.  A test of loads and stores staying inside their tensors: every run here is an
ordinary, valid call."""

import pytest
import torch

import color_ref
from color_ref import CODE, DTYPES, ELEM
from poison_util import Arena
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

POISONS = [(dt, 0xFF) for dt in sorted(DTYPES)] + [("u8", 0x00)]  # 0xFF bytes are NaN in the floating-point types; uint8 gets both
IDS = [f"{d}_{g:02x}" for d, g in POISONS]
SLOTS = _ffi.MZ_METRIC_SLOTS


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("standard", sorted(CODE))
@pytest.mark.parametrize("dt, guard", POISONS, ids=IDS)
@pytest.mark.parametrize("shape", [(1, 1), (3, 31), (2, 33), (7, 129)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_luma_touches_its_tensors_only(shape, dt, guard, standard):
    B, (H, W) = 2, shape
    x = color_ref.image(B, H, W, dt).cuda()
    want = color_ref.expected(B, H, W, dt, standard, 0)
    # dense views: the 16-byte path wherever a row holds a whole run
    arena = Arena("cuda")
    xa = arena.input(x, name="x", fill=guard)
    out = arena.output((B, 1, H, W), DTYPES[dt], fill=3, name="out")
    _ffi.luma(xa.data_ptr(), xa.stride(), out.data_ptr(), out.stride(), ELEM[dt], B, H, W, CODE[standard], 0, stream())
    arena.check()
    assert color_ref.same_bits(out, want)
    # strided views: an interleaved HWC frame in, every second column of a wider plane out (the element path on both sides)
    arena = Arena("cuda")
    xa = arena.input(x.permute(0, 2, 3, 1), name="x_hwc", fill=guard).permute(0, 3, 1, 2)
    wide = arena.output((B, 1, H, 2 * W), DTYPES[dt], fill=3, name="out_wide")
    out = wide[..., ::2]
    _ffi.luma(xa.data_ptr(), xa.stride(), out.data_ptr(), out.stride(), ELEM[dt], B, H, W, CODE[standard], 0, stream())
    arena.check()
    assert color_ref.same_bits(out, want)
    assert bool((wide[..., 1::2] == 3).all())  # the columns between keep the fill


def metrics(arena, p, t, elem, B, H, W, which, ws_fill):
    need = _ffi.metrics_luma_workspace_bytes(B, H, W, which)
    out = arena.output((B, SLOTS), torch.float64, fill=-1.0, name="out") if arena else torch.full((B, SLOTS), -1.0, dtype=torch.float64, device="cuda")
    if arena is None:
        ws = torch.full((need,), ws_fill, dtype=torch.uint8, device="cuda")
    elif ws_fill == "pattern":
        ws = arena.raw(need, 0, name="workspace")
        ws.copy_(torch.arange(need, device="cuda").mul_(37).add_(11).bitwise_and_(255).to(torch.uint8))
    else:
        ws = arena.raw(need, ws_fill, name="workspace")
    _ffi.metrics_luma(p.data_ptr(), p.stride(), t.data_ptr(), t.stride(), elem, B, H, W, which, 0, -1.0, 2.0, out.data_ptr(), ws.data_ptr(), need,
                      stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt, guard", POISONS, ids=IDS)
@pytest.mark.parametrize("shape", [(11, 11), (27, 43), (45, 52)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_luma_metrics_touch_their_tensors_only_whatever_the_workspace_holds(shape, dt, guard):
    B, (H, W) = 2, shape
    which = 7 if min(H, W) >= 41 else 3
    p = color_ref.image(B, H, W, dt, seed=8, special=False).cuda()
    t = color_ref.image(B, H, W, dt, seed=9, special=False).cuda()
    plain = metrics(None, p, t, ELEM[dt], B, H, W, which, 0)
    assert not bool(plain[:, [0, 6]].isnan().any())
    for ws_fill in (0xFF, "pattern"):  # NaN as float64, and bytes that differ from place to place
        arena = Arena("cuda")
        pa, ta = arena.input(p, name="pred", fill=guard), arena.input(t, name="target", fill=guard)
        got = metrics(arena, pa, ta, ELEM[dt], B, H, W, which, ws_fill)
        arena.check()
        assert torch.equal(got, plain), (ws_fill, got, plain)
    # strided: interleaved HWC frames
    arena = Arena("cuda")
    pa = arena.input(p.permute(0, 2, 3, 1), name="pred_hwc", fill=guard).permute(0, 3, 1, 2)
    ta = arena.input(t.permute(0, 2, 3, 1), name="target_hwc", fill=guard).permute(0, 3, 1, 2)
    got = metrics(arena, pa, ta, ELEM[dt], B, H, W, which, 0xFF)
    arena.check()
    assert torch.equal(got, plain), (got, plain)
