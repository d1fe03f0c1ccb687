"""Every conv and mix family on data that make its arithmetic exact (tests/exact_util.py): the output must equal the float64 result
rounded once to the storage type, bit for bit -- fp32 accumulation, ONE nearest-even rounding, z rounded before the gate and the blend.
No tolerance and no sibling kernel; only the elements whose gate (or SiLU) argument lies inside (SAT_LO, SAT_HI), where the
transcendental is not exact, are compared with the one-operator tolerance instead.  tests/test_exact_cpu.py holds the data to the
conditions that keep these equalities from being vacuous."""

import pytest
import torch

from exact_util import MAX_EXCLUDED, ROWS, WALKS, bits_of, exact, row_id, walk_id
from gpu_util import DTYPES, alloc_act, assert_op_close, last_kernel, pad_part, to_act
from op_util import run_entry, set_knobs

pytestmark = pytest.mark.gpu

ACTIVATIONS = {"in0", "in1", "hid", "x", "feat"}  # plane-major activation tensors; the stem's x and the head's img are dense images


def launch(row, ex):
    """The row's operator on the row's data: (output on the GPU, its real channels [B, C, H, W] on the CPU, storage type)."""
    dtype = DTYPES[row.dt]
    t = {}
    for name, v in ex.inputs.items():
        if name in ACTIVATIONS and not (row.entry == "stem" and name == "x"):
            t[name] = to_act(v, dtype)
        elif name in ("x", "img"):
            t[name] = v.to("cuda", dtype).contiguous()
        else:
            t[name] = v.to("cuda", torch.float32).contiguous()
    B = row.args[0]
    if ex.C is None:
        out = torch.full(tuple(ex.want.shape), 7.0, dtype=dtype, device="cuda")
    else:
        out = alloc_act(B, ex.C, ex.want.shape[2], ex.want.shape[3], dtype)
    run_entry(row.entry, row.args, row.dt, t, out, ex.alpha)
    if ex.C is None:
        return out, out.cpu()
    Bo, P, H, W, ppu = out.shape
    return out, out.permute(0, 1, 4, 2, 3).reshape(Bo, P * ppu, H, W)[:, :ex.C].cpu()


def check(row, ex, out, got):
    if row.kernel is not None:
        assert last_kernel() == row.kernel, (last_kernel(), row.kernel)
    want = ex.want
    assert got.shape == want.shape and got.dtype == want.dtype
    g, w = (got, want) if ex.keep is None else (got[ex.keep], want[ex.keep])
    if not torch.equal(g, w):
        bad = (got != want) if ex.keep is None else (got != want) & ex.keep
        idx = tuple(int(v) for v in bad.nonzero()[0])
        mask = 0xFFFFFFFF if row.dt == "f32" else 0xFFFF
        raise AssertionError(f"{row_id(row)}: {int(bad.sum())} of {g.numel()} elements differ from the float64 result rounded once; first at "
                             f"{idx}: got {got[idx].item()!r} (bits {bits_of(got[idx].reshape(1)).item() & mask:#x}), want "
                             f"{want[idx].item()!r} (bits {bits_of(want[idx].reshape(1)).item() & mask:#x}), float64 {ex.y64[idx].item()!r}")
    if ex.keep is not None:
        print(f"{row_id(row)}: excluded share {ex.excluded:.5f} ({int((~ex.keep).sum())} elements)")
        assert ex.excluded <= MAX_EXCLUDED
        assert bool(torch.isfinite(got.float()).all())
        soft = ~ex.keep
        if bool(soft.any()):
            assert_op_close(got.float()[soft], ex.soft64[soft].float(), row.dt, row_id(row) + " (excluded elements)")
    if ex.C is not None:
        assert bool((pad_part(out, ex.C) == 0).all()), "pad channels must be written as zeros"


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_bit_for_bit(row, monkeypatch):
    set_knobs(monkeypatch, row.env)
    ex = exact(row)
    out, got = launch(row, ex)
    check(row, ex, out, got)


@pytest.mark.parametrize("walk", WALKS, ids=walk_id)
def test_bit_for_bit_persistent_walks(walk, monkeypatch):
    """The same row with 8 and with 16 persistent workgroups: each run equals the expectation, not merely the other run."""
    row, wgs = walk
    set_knobs(monkeypatch, row.env, wgs)
    ex = exact(row)
    out, got = launch(row, ex)
    check(row, ex, out, got)
