"""mz_dihedral and the mz_ensemble_add / mz_ensemble_finish sequence in poisoned surroundings (tests/poison_util.py), in the manner of
tests/test_poison_resize_gpu.py: the input between NaN guards (uint8: 0xFF and 0x00 guards), the output between pattern guards, the
accumulator workspace pre-filled with 0xFF bytes (NaN as float32) between pattern guards.  The results have the bits of the run on
ordinary tensors, no guard and no input has changed.  A test of loads and stores staying inside their tensors: every run here is an
ordinary, valid call."""

import pytest
import torch

import ensemble_ref as ref
from ensemble_ref import DTYPES, pass_results, random_bits, shape_id, stream
from poison_util import Arena
from ultrazoom_amd import _ffi, dihedral

pytestmark = pytest.mark.gpu

SHAPES = [(2, 31, 33), (1, 65, 127)]
KS = [0, 3, 5, 7]
POISONS = [(dt, 0xFF) for dt in sorted(DTYPES)] + [("u8", 0x00)]  # 0xFF bytes are NaN in the floating-point types; uint8 gets both


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dt, guard", POISONS, ids=[f"{d}_{g:02x}" for d, g in POISONS])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_dihedral_touches_its_tensors_only(shape, dt, guard, k):
    B, H, W = shape
    x = random_bits(dt, B, H, W, seed=1)
    want = dihedral(x, k)
    arena = Arena("cuda")
    xa = arena.input(x, name="x", fill=guard)
    out = arena.output(tuple(want.shape), DTYPES[dt], fill=3, name="out")
    _ffi.dihedral(xa.data_ptr(), xa.stride(), out.data_ptr(), out.stride(), _ffi.elem_code(DTYPES[dt]), B, H, W, k, stream())
    arena.check()
    assert torch.equal(ref.bits(out), ref.bits(want))
    assert torch.equal(ref.bits(out), ref.bits(ref.T(x, k)))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dt, guard", POISONS, ids=[f"{d}_{g:02x}" for d, g in POISONS])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_add_and_finish_touch_their_tensors_only(shape, dt, guard, k):
    """Two results -- orientation k stored, orientation inverse(k) ^ 1 added -- and the finish of n = 2."""
    B, H, W = shape
    dtype, elem = DTYPES[dt], _ffi.elem_code(DTYPES[dt])
    ys = pass_results(dt, B, H, W)
    order = [k, ref.inverse(k) ^ 1]
    need = _ffi.ensemble_workspace_bytes(B, H, W)

    def sequence(inputs, ws, out):
        for i, (kk, y) in enumerate(zip(order, inputs)):
            _ffi.ensemble_add(y.data_ptr(), y.stride(), elem, B, H, W, kk, i == 0, ws.data_ptr(), need, stream())
        _ffi.ensemble_finish(out.data_ptr(), out.stride(), elem, B, H, W, 2, 1, None, ws.data_ptr(), need, stream())

    plain_ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    plain = torch.empty((B, 3, H, W), dtype=dtype, device="cuda")
    sequence([ys[kk] for kk in order], plain_ws, plain)

    arena = Arena("cuda")
    inputs = [arena.input(ys[kk], name=f"y{i}", fill=guard) for i, kk in enumerate(order)]
    out = arena.output((B, 3, H, W), dtype, fill=3, name="out")
    ws = arena.raw(need, 0xFF, name="workspace")
    sequence(inputs, ws, out)
    arena.check()
    if dt != "u8":
        assert not bool(torch.isnan(out).any())
    assert torch.equal(ref.bits(out), ref.bits(plain))
    assert torch.equal(ws, plain_ws), "the accumulator depends on what the workspace held"
    assert torch.equal(ref.bits(out), ref.bits(ref.finish(ref.accumulate([ys[kk] for kk in order], order), 2, dtype, True)))
