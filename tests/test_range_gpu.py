"""Every conv and mix family at the ends of its storage type and across the window of its transcendentals (tests/range_util.py):

  small   data at the BOTTOM of the type, subnormal inputs and results: the output equals the float64 result rounded once, bit for bit;
  large   f16 outputs that straddle 65504: the same equality, +-inf from the tie 65520 upward;
  window  SiLU and the gate's blend on every finite value of the type inside (-100, 32), against float64 within
          0.5 ulp + 2^-16 scale + 2^-126 (no absolute floor; range_util.RCP_MIN: where sigmoid(t) < 2^-126 the result may be the one
          with the sigmoid taken as zero), and bit for bit between the families that promise identical bits.

tests/test_range_cpu.py holds the data to the conditions that keep these from being vacuous."""

import pytest
import torch

from exact_util import MAX_EXCLUDED, bits_of, row_id
from gpu_util import DTYPES, alloc_act, assert_op_close, last_kernel, pad_part, to_act
from op_util import run_entry, set_knobs
from range_util import GATE_WINDOW, LARGE, SILU_TWINS, SILU_WINDOW, SMALL, large, small, small_id, win_id, window, window_ratio

pytestmark = pytest.mark.gpu

ACTIVATIONS = {"in0", "in1", "hid", "x", "feat"}  # plane-major activation tensors; the stem's x and the head's img are dense images


def launch(entry, args, dt, inputs, C, shape, alpha=0.0):
    """The operator on the given data: (output on the GPU, its real channels [B, C, H, W] on the CPU, storage type)."""
    dtype = DTYPES[dt]
    t = {}
    for name, v in inputs.items():
        if name in ACTIVATIONS and not (entry == "stem" and name == "x"):
            t[name] = to_act(v, dtype)
        elif name in ("x", "img"):
            t[name] = v.to("cuda", dtype).contiguous()
        else:
            t[name] = v.to("cuda", torch.float32).contiguous()
    if C is None:
        out = torch.full(tuple(shape), 7.0, dtype=dtype, device="cuda")
    else:
        out = alloc_act(shape[0], C, shape[2], shape[3], dtype)
    run_entry(entry, args, dt, t, out, alpha)
    if C is None:
        return out, out.cpu()
    Bo, P, H, W, ppu = out.shape
    return out, out.permute(0, 1, 4, 2, 3).reshape(Bo, P * ppu, H, W)[:, :C].cpu()


def check(row, what, ex, out, got):
    """Equality with the float64 result rounded once (zeros of either sign are equal); exact_util's rule for the excluded elements."""
    if row.kernel is not None:
        assert last_kernel() == row.kernel, (last_kernel(), row.kernel)
    want = ex.want
    assert got.shape == want.shape and got.dtype == want.dtype
    assert not bool(torch.isnan(got.float()).any())
    g, w = (got, want) if ex.keep is None else (got[ex.keep], want[ex.keep])
    if not torch.equal(g, w):
        bad = (got != want) if ex.keep is None else (got != want) & ex.keep
        idx = tuple(int(v) for v in bad.nonzero()[0])
        mask = 0xFFFFFFFF if row.dt == "f32" else 0xFFFF
        flushed = int((bad & (got == 0)).sum())
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ from the float64 result rounded once ({flushed} of them are "
                             f"zero); first at {idx}: got {got[idx].item()!r} (bits {bits_of(got[idx].reshape(1)).item() & mask:#x}), want "
                             f"{want[idx].item()!r} (bits {bits_of(want[idx].reshape(1)).item() & mask:#x}), float64 {ex.y64[idx].item()!r}")
    if ex.keep is not None:
        assert ex.excluded <= MAX_EXCLUDED
        assert bool(torch.isfinite(got.float()).all())
        soft = ~ex.keep
        if bool(soft.any()):
            assert_op_close(got.float()[soft], ex.soft64[soft].float(), row.dt, what + " (excluded elements)")
    if ex.C is not None:
        assert bool((pad_part(out, ex.C) == 0).all()), "pad channels must be written as zeros"


@pytest.mark.parametrize("s", SMALL, ids=small_id)
def test_small_bit_for_bit(s, monkeypatch):
    row = s.row
    set_knobs(monkeypatch, row.env)
    ex = small(s)
    out, got = launch(row.entry, row.args, row.dt, ex.inputs, ex.C, ex.want.shape, ex.alpha)
    check(row, small_id(s), ex, out, got)


@pytest.mark.parametrize("row", LARGE, ids=row_id)
def test_large_bit_for_bit(row, monkeypatch):
    set_knobs(monkeypatch, row.env)
    ex = large(row)
    out, got = launch(row.entry, row.args, row.dt, ex.inputs, ex.C, ex.want.shape)
    check(row, row_id(row) + "-large", ex, out, got)
    assert bool(torch.isinf(got).any())


def sweep(w, monkeypatch):
    set_knobs(monkeypatch, w.env)
    wd = window(w)
    out, got = launch(w.entry, w.args, w.dt, wd.inputs, wd.C, wd.want64.shape)
    assert last_kernel() == w.kernel, (last_kernel(), w.kernel)
    assert bool((pad_part(out, wd.C) == 0).all()), "pad channels must be written as zeros"
    return wd, got


def within(w, wd, got):
    assert bool(torch.isfinite(got.float()).all())
    ratio = window_ratio(got, wd.want64, wd.scale64, w.dt, wd.may_flush, wd.flushed64)
    worst = int(ratio.argmax())
    x = wd.x64.flatten()[worst].item()
    print(f"window {w.kernel} {win_id(w)}: worst |got - want| / bound {ratio.max().item():.4f} at x = {x!r}")
    bad = ratio > 1.0
    assert not bool(bad.any()), (f"{win_id(w)}: {int(bad.sum())} of {bad.numel()} elements miss 0.5 ulp + 2^-16 scale + 2^-126; the worst, "
                                 f"{ratio.max().item():.3f} x the bound, at x = {x!r}: got {got.flatten()[worst].item()!r}, want "
                                 f"{wd.want64.flatten()[worst].item()!r}; {int((bad & (got == 0)).sum())} of them are zero")


@pytest.mark.parametrize("w", SILU_WINDOW, ids=win_id)
def test_window_silu(w, monkeypatch):
    """SiLU(t) of t exactly as stored (one-hot weights), every value of the type inside the window."""
    wd, got = sweep(w, monkeypatch)
    within(w, wd, got)


@pytest.mark.parametrize("w", GATE_WINDOW, ids=win_id)
def test_window_gate(w, monkeypatch):
    """x + sigmoid(x) (z - x) / 2: the gate's weights are one-hot on x, alpha = 0, z a fixed permutation of the same values."""
    wd, got = sweep(w, monkeypatch)
    within(w, wd, got)


@pytest.mark.parametrize("pair", SILU_TWINS, ids=lambda pq: f"{win_id(pq[0])}-{pq[1].kernel}")
def test_window_silu_identical_bits(pair, monkeypatch):
    """Families whose SiLU is "the same operations in the same order" (mz_relay.h, mz_conv3r.h) on the same input: the same bits."""
    (_, a), (_, b) = sweep(pair[0], monkeypatch), sweep(pair[1], monkeypatch)
    same = bits_of(a) == bits_of(b)
    assert bool(same.all()), f"{int((~same).sum())} of {same.numel()} elements differ between {pair[0].kernel} and {pair[1].kernel}"
