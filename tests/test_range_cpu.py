"""The number-range tables (tests/range_util.py) held to the conditions that keep tests/test_range_gpu.py from being vacuous, with the
float64 reference alone: no GPU.  These are conditions on the test data, not measurements of a kernel."""

import math

import numpy as np
import pytest
import torch

from exact_util import EXACT_SUM, MAX_EXCLUDED, MIN_BRANCH, ROWS, SAT_HI, SAT_LO, bits_of, lower_edge, round_once, row_id
from gpu_util import DTYPES, ulp_of
from op_cases import CASES, FAMILY_OF_UNREPORTED, TINY_CASES
from op_util import kernel_names, selected, set_knobs
from range_util import (F16_MAX, F16_TIE, FLOOR_W, FLOOR_X, FLUSH, GATE_SHIFT, GATE_WINDOW, LARGE, MIN_NORMAL, MIN_SUB_INEXACT, MIN_SUB_SHARE, MIN_SUB_TIES, REL,
                        RCP_MIN, SILU_TWINS, SILU_WINDOW, SMALL, STORE_ENTRIES, VARIANTS, is_sub, large, lean, small, small_id, sub_census, ulp64, win_id, window,
                        window_ratio, window_values)


def as_torch(y64, dt):
    """torch's own conversion, for values that float32 holds exactly (so that float64 -> float32 -> dt rounds once)."""
    assert torch.equal(y64.float().double(), y64), "a reference value is no float32"
    return y64.float().to(DTYPES[dt])


def same_bits(a, b):
    return torch.equal(bits_of(a), bits_of(b))


def data_rows(rows, key):
    return list({key(r): r for r in rows}.values())  # rows that differ in their knobs share their data


# ---- SMALL ---------------------------------------------------------------------------------------------------------------------------
DATA_SMALL = data_rows(SMALL, lambda s: (s.row.entry, s.row.args, s.row.dt, s.row.silu, s.variant))


@pytest.mark.parametrize("s", DATA_SMALL, ids=small_id)
def test_the_small_row_s_conditions(s):
    row, dt, ex = s.row, s.row.dt, small(s)
    # every reference value is a float32 (an exact fp32 accumulation can hold it), and round_once is torch's conversion on them
    assert same_bits(ex.want, as_torch(ex.y64, dt))
    if hasattr(ex, "z64_unrounded"):
        assert same_bits(round_once(ex.z64_unrounded, dt), as_torch(ex.z64_unrounded, dt))
    for name, v in ex.sums.items():
        assert v < EXACT_SUM, f"{name}: a sum of absolute products reaches {v:.0f} >= 2^24 grid units"
    for name, t in ex.inputs.items():
        if name in ("gamma", "beta", "b") or (row.entry == "stem" and name == "w"):
            continue  # per-channel f32 parameters
        assert same_bits(t.to(DTYPES[dt]).float(), t), f"{name} is not a value of the storage type"
    # the variant's stated share of its inputs is subnormal
    assert ex.subnormal, "the variant states no subnormal input"
    for name, (share, floor) in ex.subnormal.items():
        assert floor in (FLOOR_X, FLOOR_W) and share >= floor, f"{name}: {share:.4f} of it is subnormal, the floor is {floor}"
    if ex.keep is not None:
        assert ex.excluded <= MAX_EXCLUDED, f"excluded share {ex.excluded:.4f}"
        assert min(ex.branches) >= MIN_BRANCH, ex.branches
    if row.entry in ("mix", "conv_mix"):
        assert ex.gate_shift <= GATE_SHIFT, f"the channels that are no drivers move a gate by up to {ex.gate_shift:.3e}"
        assert not bool(ex.z64[:, ~ex.rest].any()), "z is not zero in a driver channel"
    if row.silu:
        # saturated SiLU (range_util's docstring): the outputs are t or 0, the subnormals are the activations
        assert ex.keep is not None and "in0" in ex.subnormal
        return
    # the census, among compared outputs; a mix's driver channels are there to drive and are left out of it
    if row.entry in ("mix", "conv_mix"):
        keep = ex.keep & ex.rest[None, :, None, None]
        y = ex.y64[keep]
    else:
        y = ex.compared()
    share, inexact, ties, up = sub_census(y, dt)
    if dt == "f32":
        assert bool((y.abs() < MIN_NORMAL[dt]).all()) and share >= 0.5, f"f32: {share:.3f} of the outputs are non-zero subnormals"
        assert inexact == 0
        return
    assert share >= MIN_SUB_SHARE, f"{share:.3f} of the outputs are subnormal"
    assert up >= 1, "no subnormal output tells truncation from nearest-even"
    if lean(s):
        assert any(o.variant == s.variant and o.row.entry == row.entry and o.row.kernel == row.kernel and o.row.dt == dt and not lean(o) for o in SMALL), \
            "no row of ordinary size"
        return
    assert inexact >= MIN_SUB_INEXACT, f"{inexact} subnormal outputs need rounding"
    assert ties >= MIN_SUB_TIES, f"{ties} exact ties in the subnormal range"


def test_the_gate_s_margins():
    """What GATE_SHIFT may move a driver-only gate by changes neither saturated branch."""
    assert math.exp(-(SAT_HI - GATE_SHIFT)) < 2.0 ** -46  # vanishes beside 1 in fp32
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(math.exp(-(SAT_LO + GATE_SHIFT))))  # e^-t still overflows fp32


def test_the_small_table_covers_the_exact_table():
    ordinary = [r for r in ROWS if not lower_edge(r)]
    for r in ordinary:
        want = [v for v in VARIANTS[r.dt] if not (v == "wsub" and (r.entry in ("mix", "stem") or r.silu))]
        assert [s.variant for s in SMALL if s.row == r] == want, row_id(r)
    assert len({small_id(s) for s in SMALL}) == len(SMALL)
    named = {(s.row.entry, s.row.args, s.variant) for s in SMALL if lean(s)}
    assert all(n < 10000 for n in (small(s).y64.numel() for s in SMALL if lean(s))), "a row of ordinary size is exempt"
    assert named


# ---- LARGE ---------------------------------------------------------------------------------------------------------------------------
DATA_LARGE = data_rows(LARGE, lambda r: (r.entry, r.args))


@pytest.mark.parametrize("row", DATA_LARGE, ids=row_id)
def test_the_large_row_s_conditions(row):
    ex = large(row)
    assert same_bits(ex.want, as_torch(ex.y64, "f16"))
    for name, v in ex.sums.items():
        assert v < EXACT_SUM, f"{name}: a sum of absolute products reaches {v:.0f} >= 2^24"
    for name, t in ex.inputs.items():
        if name in ("gamma", "beta", "b") or (row.entry == "stem" and name == "w"):
            continue
        assert same_bits(t.half().float(), t), f"{name} is not a value of the storage type"
    y, w = ex.y64, ex.want.double()
    inf = torch.isinf(w)
    assert torch.equal(inf, y.abs() >= F16_TIE)
    share = inf.double().mean().item()
    assert 0.05 <= share <= 0.5, f"{share:.3f} of the outputs are infinite"
    assert bool((w == math.inf).any()) and bool((w == -math.inf).any())
    assert int(((y.abs() >= 32768.0) & ~inf).sum()) >= 100
    # the constructed elements: the tie that rounds to +inf, the value just below it (65504), the negative tie
    for v, to in ((F16_TIE, math.inf), (F16_TIE - 1.0, F16_MAX), (-F16_TIE, -math.inf)):
        at = y == v
        assert bool(at.any()), f"no output is exactly {v}"
        assert bool((w[at] == to).all())


def test_the_large_table_covers_the_f16_store_rows():
    assert LARGE == [r for r in ROWS if not lower_edge(r) and r.dt == "f16" and r.entry in STORE_ENTRIES and not r.silu]
    assert {r.entry for r in LARGE} == set(STORE_ENTRIES)


# ---- WINDOW --------------------------------------------------------------------------------------------------------------------------
def patterns(t, dt):
    return set(bits_of(t.to(DTYPES[dt]).flatten()).tolist())


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_the_window_s_values(dt):
    v = window_values(dt)
    assert bool(((v > SAT_LO) & (v < SAT_HI)).all())
    assert len(patterns(v, dt)) == v.numel()  # distinct bit patterns: +0 and -0 both
    assert int((v == 0).sum()) == 2 and bool(torch.signbit(v[v == 0]).any())
    if dt == "f32":
        assert patterns(window_values("bf16"), "f32") | patterns(window_values("f16"), "f32") == patterns(v, "f32")
        return
    # counted on the bit patterns: [+0, 32) and [-0, -100) are two runs of consecutive patterns
    hi, lo = torch.tensor([SAT_HI, -SAT_LO], dtype=DTYPES[dt]).view(torch.int16).tolist()
    assert v.numel() == hi + lo == {"bf16": 33992, "f16": 42560}[dt]
    assert int(is_sub(v, dt).sum()) == 2 * ((1 << {"bf16": 7, "f16": 10}[dt]) - 1)  # every subnormal of the type


@pytest.mark.parametrize("w", SILU_WINDOW + GATE_WINDOW, ids=win_id)
def test_the_window_row_sweeps_every_value(w, monkeypatch):
    wd = window(w)
    for name, t in wd.inputs.items():
        if name not in ("gamma", "beta"):
            assert same_bits(t.to(DTYPES[w.dt]).float(), t), f"{name} is not a value of the storage type"
    assert patterns(window_values(w.dt), w.dt) <= patterns(wd.read, w.dt), "a value of the window is missing from the channels that are read"
    assert patterns(wd.x64.float(), w.dt) == patterns(wd.read, w.dt), "an output's argument is none of the values that are read"
    assert bool(((wd.x64 > SAT_LO) & (wd.x64 < SAT_HI)).all())
    if w.dt == "f32":  # and random bit patterns beside the two 16-bit sets
        assert len(patterns(wd.read, "f32")) >= 1.15 * window_values("f32").numel()
    if w.entry in ("mix", "conv_mix"):
        assert torch.equal(wd.x64.flatten().sort().values, wd.z64.flatten().sort().values) and not torch.equal(wd.x64, wd.z64)
    # the identity: one-hot weights
    for name in ("w", "w2", "wmix"):
        if name in wd.inputs:
            t = wd.inputs[name]
            assert bool(((t == 0) | (t == 1)).all()) and bool((t.flatten(1).sum(1) == 1).all())
    set_knobs(monkeypatch, w.env)
    assert selected(w.entry, w.args, w.dt) == w.kernel


def test_the_window_bound():
    """0.5 ulp + 2^-16 scale + 2^-126, on constructed values; ulp64 against gpu_util.ulp_of."""
    for dt in ("bf16", "f16"):
        v = window_values(dt)
        assert torch.equal(ulp64(v.double(), dt), ulp_of(v, dt).double())
    assert ulp64(torch.tensor([0.0, 2.0 ** -149, 1.0, 1.5, 2.0], dtype=torch.float64), "f32").tolist() == [2.0 ** -149, 2.0 ** -149, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
    want = torch.tensor([1.0, 1.0, 0.0, 2.0 ** -20], dtype=torch.float64)
    got = want + torch.tensor([2.0 ** -11 + 2.0 ** -16, 2.0 ** -10, 2.0 ** -25, 2.0 ** -24], dtype=torch.float64)
    r = window_ratio(got, want, want.abs(), "f16")
    assert r[0] <= 1.0 < r[1] and r[2] <= 1.0 < r[3], r  # no absolute floor: half a subnormal spacing passes, a whole one does not
    assert REL == 2.0 ** -16 and FLUSH == 2.0 ** -126 and 2.0 * (100 * 2.0 ** -24 + 3 * 2.0 ** -24) <= REL


def test_the_reciprocal_s_flush_is_admitted_only_below_its_threshold():
    """range_util.RCP_MIN: a zero sigmoid passes only where the true one lies below 2^-126 (t < -87.33), and nothing else passes there."""
    w = next(w for w in SILU_WINDOW if w.dt == "bf16")
    wd = window(w)
    assert bool((wd.x64[wd.may_flush] < -87.33).all()) and bool((wd.x64[~wd.may_flush] > -87.34).all())
    band = wd.may_flush & (wd.want64.abs() > 2.0 * RCP_MIN)
    assert int(band.sum()) >= 5, "no value of the window meets the flush"
    flushed = torch.where(wd.x64 < -80.0, 0.0 * wd.want64, wd.want64)
    r = window_ratio(flushed, wd.want64, wd.scale64, w.dt, wd.may_flush, wd.flushed64)
    assert bool((r[band] <= 1.0).all()) and bool((r[(wd.x64 < -80.0) & ~wd.may_flush] > 1.0).all())
    assert bool((window_ratio(flushed, wd.want64, wd.scale64, w.dt)[band] > 1.0).all())  # the bound alone does not admit it
    r = window_ratio(0.5 * wd.want64, wd.want64, wd.scale64, w.dt, wd.may_flush, wd.flushed64)
    assert bool((r[band] > 1.0).all())
    g = window(next(w for w in GATE_WINDOW if w.dt == "bf16"))
    assert bool((g.x64[g.may_flush] < -86.6).all()) and bool(g.may_flush.any()) and torch.equal(g.flushed64, g.x64)


def test_the_tables_name_every_kernel_family():
    """Every literal kernel_name() (mz_select.h) can return has a small row; every family that applies SiLU a window row; every gated
    family a gate row."""
    names = kernel_names()
    covered = {s.row.kernel for s in SMALL if s.row.kernel} | {FAMILY_OF_UNREPORTED[s.row.entry] for s in SMALL if s.row.entry in FAMILY_OF_UNREPORTED}
    assert names <= covered, f"no small row runs {sorted(names - covered)}"
    for dt in ("bf16", "f16", "f32"):
        for v in VARIANTS[dt]:
            have = {s.row.kernel for s in SMALL if s.row.dt == dt and s.variant == v}
            # (the mix entry has no weights but its gate's: no "wsub" variant, range_util's docstring)
            assert {r.kernel for r in ROWS if r.dt == dt and r.kernel and not r.silu and not (v == "wsub" and r.entry == "mix")} <= have, (dt, v)
    tiny = {(e, a) for e, a, _, _, _ in TINY_CASES}
    silu = {k for e, a, _, _, k in CASES if e in ("conv", "film") and (e, a) not in tiny}
    assert silu <= {w.kernel for w in SILU_WINDOW}, f"no SiLU window row runs {sorted(silu - {w.kernel for w in SILU_WINDOW})}"
    assert any(w.entry == "film" for w in SILU_WINDOW)
    gated = {n for n in names if n.endswith(("_mix", "_fused"))} | {"mix16", "mix16b"}
    assert gated <= {w.kernel for w in GATE_WINDOW}
    for dt in ("bf16", "f16"):
        assert gated <= {w.kernel for w in GATE_WINDOW if w.dt == dt}
    # the families that promise identical bits are compared with each other
    assert {frozenset((p.kernel, q.kernel)) for p, q in SILU_TWINS} >= {frozenset(("conv3r", "conv3s")), frozenset(("conv3r_8x40", "conv3s")), frozenset(("conv3t", "conv3s"))}
