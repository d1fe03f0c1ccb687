"""Every conv and mix family at the ends of its storage type and across the window of its transcendentals (tests/range_util.py):

  small   data at the BOTTOM of the type, subnormal inputs and results: the output equals the float64 result rounded once, bit for bit;
  large   f16 outputs that straddle 65504: the same equality, +-inf from the tie 65520 upward;
  window  SiLU and the gate's blend on every finite value of the type inside (-100, 32), against float64 within
          0.5 ulp + 2^-16 scale + 2^-126 (no absolute floor; range_util.RCP_MIN: where sigmoid(t) < 2^-126 the result may be the one
          with the sigmoid taken as zero), and bit for bit between the families that promise identical bits.

tests/test_range_cpu.py holds the data to the conditions that keep these from being vacuous."""

import pytest
import torch

from exact_util import bits_of, row_id
from gpu_util import last_kernel, pad_part
from op_util import check_rounded_once, launch, set_knobs
from range_util import GATE_WINDOW, LARGE, SILU_TWINS, SILU_WINDOW, SMALL, large, small, small_id, win_id, window, window_ratio

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("s", SMALL, ids=small_id)
def test_small_bit_for_bit(s, monkeypatch):
    row = s.row
    set_knobs(monkeypatch, row.env)
    ex = small(s)
    out, got = launch(row.entry, row.args, row.dt, ex.inputs, ex.alpha)
    check_rounded_once(row, small_id(s), ex, out, got)


@pytest.mark.parametrize("row", LARGE, ids=row_id)
def test_large_bit_for_bit(row, monkeypatch):
    set_knobs(monkeypatch, row.env)
    ex = large(row)
    out, got = launch(row.entry, row.args, row.dt, ex.inputs)
    check_rounded_once(row, row_id(row) + "-large", ex, out, got)
    assert bool(torch.isinf(got).any())


def sweep(w, monkeypatch):
    set_knobs(monkeypatch, w.env)
    wd = window(w)
    out, got = launch(w.entry, w.args, w.dt, wd.inputs)
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
