"""The exact-arithmetic table (tests/exact_util.py) held to the conditions that keep tests/test_exact_gpu.py from being vacuous, with
the float64 reference alone: no GPU.  These are conditions on the test data, not measurements of a kernel."""

import pytest
import torch

from exact_util import (CENSUS_MIN, CENSUS_MIN_SHARE, EXACT_SUM, F16_MAX_OUT, MAX_EXCLUDED, MIN_BRANCH, PERSISTENT, ROWS, WALK_WGS, WALKS, bits_of, census, exact, lower_edge, round_once, row_id,
                        walk_id)
from gpu_util import DTYPES
from op_cases import FAMILY_OF_UNREPORTED, select_args
from op_util import kernel_names, selected, set_knobs


def as_torch(y64, dt):
    """torch's own conversion, for values that float32 holds exactly (so that float64 -> float32 -> dt rounds once)."""
    assert torch.equal(y64.float().double(), y64)
    return y64.float().to(DTYPES[dt])


def same_bits(a, b):
    return torch.equal(bits_of(a), bits_of(b))


def neighbours(v, dt):
    """The `dt` value v and the next one away from zero, as float64."""
    t = torch.tensor([v], dtype=DTYPES[dt])
    assert t.double().item() == v
    return v, (bits_of(t) + 1).view(DTYPES[dt]).double().item()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_round_once_at_constructed_ties(dt):
    """Halfway between two neighbours, below an even and below an odd one, both signs, and a hair to either side of the tie."""
    ys = []
    for v in (1.0, 3.0, 256.0, 2048.0, 1000.0, 0.15625):
        for lo in (v, neighbours(v, dt)[1]):  # the mantissa of v is even, that of its successor odd
            lo, hi = neighbours(lo, dt)
            mid, eps = (lo + hi) / 2, (hi - lo) / 1024  # (exact in float32 for bf16 / f16; f32: eps is dropped below)
            ys += [mid, -mid, lo, hi] + ([mid - eps, mid + eps, -mid - eps] if dt != "f32" else [])
    y = torch.tensor(ys, dtype=torch.float64)
    if dt == "f32":  # torch rounds float64 -> float32 once, by the hardware's conversion
        assert same_bits(round_once(y, dt), y.float())
    else:
        assert same_bits(round_once(y, dt), as_torch(y, dt))
    need, tie, up = census(y, dt)
    assert tie > 0 and need >= tie and 0 < up < need
    # a tie goes to the even neighbour: below an even mantissa down, below an odd one up
    lo, hi = neighbours(1.0, dt)
    assert round_once(torch.tensor([(lo + hi) / 2], dtype=torch.float64), dt).double().item() == lo
    lo2, hi2 = neighbours(hi, dt)
    assert round_once(torch.tensor([(lo2 + hi2) / 2], dtype=torch.float64), dt).double().item() == hi2


def test_round_once_at_the_f16_subnormal_edge():
    """f16: subnormals are multiples of 2^-24 below 2^-14; the largest finite value is 65504, 65520 is the tie that rounds to infinity."""
    u = 2.0 ** -24
    ys = [0.0, u, u / 2, 1.5 * u, 2.5 * u, 0.75 * u, u / 4, 1023 * u, 1023.5 * u, 1024 * u, 1024.5 * u, 1025 * u, 2.0 ** -14 - u / 2,
          65504.0, 65519.0, 65520.0, 1e6]
    y = torch.tensor(ys + [-v for v in ys[1:]], dtype=torch.float64)
    got = round_once(y, "f16")
    assert same_bits(got, as_torch(y, "f16"))
    assert got[ys.index(u / 2)].item() == 0.0 and got[ys.index(1.5 * u)].double().item() == 2 * u  # ties to even
    assert torch.isinf(got[ys.index(65520.0)]) and got[ys.index(65519.0)].item() == 65504.0
    # bf16 and f32 share float32's exponent range: their subnormal edge, too
    t = 2.0 ** -126
    y = torch.tensor([t, t / 2, t * (1 + 2.0 ** -8), t * (1 - 2.0 ** -9), 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134], dtype=torch.float64)
    assert same_bits(round_once(y, "bf16"), as_torch(y, "bf16"))


DATA_ROWS = list({(r.entry, r.args, r.dt, r.silu): r for r in ROWS}.values())  # rows that differ in their knobs share their data


@pytest.mark.parametrize("row", DATA_ROWS, ids=row_id)
def test_the_row_s_conditions(row):
    ex = exact(row)
    dt = row.dt
    # round_once against torch on the row's own reference values (integers and halves below 2^24: float32 holds them)
    assert same_bits(ex.want, as_torch(ex.y64, dt))
    for name, s in ex.sums.items():
        assert s < EXACT_SUM, f"{name}: a sum of absolute products reaches {s:.0f} >= 2^24"
    for t in ex.inputs.values():
        assert same_bits(t.to(DTYPES[dt]).float(), t), "an input is not a value of the storage type"
    if dt == "f16":
        assert ex.y64.abs().max().item() < F16_MAX_OUT
        if hasattr(ex, "z64_unrounded"):
            assert ex.z64_unrounded.abs().max().item() < F16_MAX_OUT
    y = ex.compared()
    if dt != "f32" and lower_edge(row) and y.numel() < CENSUS_MIN:
        # too few elements for 100 ties (exact_util.LOWER_EDGE): the family's ties are pinned by a row of ordinary size, held to them below
        assert any(r.kernel == row.kernel and r.dt == dt and r.entry == row.entry and not lower_edge(r) for r in ROWS), "no row of ordinary size"
        if y.numel() >= CENSUS_MIN_SHARE:
            need, _, up = census(y, dt)
            assert need >= (0.20 if dt == "bf16" else 0.01), f"need rounding: {need:.4f}"
            assert up > 0, "no element tells truncation from rounding"
    elif dt != "f32":
        need, tie, up = census(y, dt)
        assert tie >= 0.01 and tie * y.numel() >= 100, f"ties: {tie:.4f} of {y.numel()}"
        assert need >= (0.20 if dt == "bf16" else 0.01), f"need rounding: {need:.4f}"
        assert up > 0, "no element tells truncation from rounding"
    if ex.keep is not None:
        assert ex.excluded <= MAX_EXCLUDED, f"excluded share {ex.excluded:.4f}"
        assert min(ex.branches) >= MIN_BRANCH, ex.branches
    if row.entry == "conv_mix" and dt != "f32":  # z itself is a rounded value: blending the unrounded one would show
        need, tie, _ = census(ex.z64_unrounded, dt)
        assert need >= 0.20 if dt == "bf16" else need >= 0.01


def test_the_table_names_every_kernel_family():
    """Every literal kernel_name() (mz_select.h) can return is the pinned family of some row."""
    names = kernel_names()
    covered = {r.kernel for r in ROWS if r.kernel} | {FAMILY_OF_UNREPORTED[r.entry] for r in ROWS if r.entry in FAMILY_OF_UNREPORTED}
    assert names <= covered, f"no row runs {sorted(names - covered)}"
    assert PERSISTENT <= names
    assert len({row_id(r) for r in ROWS}) == len(ROWS)
    # every dtype of every family ending in _mix or _fused, and both 16-bit mix kernels
    gated = {n for n in names if n.endswith(("_mix", "_fused"))} | {"mix16", "mix16b"}
    assert gated <= {r.kernel for r in ROWS if r.entry in ("mix", "conv_mix")}


def choice_of(row, monkeypatch, wgs=None):
    set_knobs(monkeypatch, row.env, wgs)
    return selected(row.entry, row.args, row.dt, row.silu)


@pytest.mark.parametrize("row", [r for r in ROWS if select_args(r.entry, r.args) is not None], ids=row_id)
def test_the_pinned_families_are_the_host_s_choice(row, monkeypatch):
    """With SiLU off, and for this table's own shapes: the name of every row is what the host chooses on an MI355X (256 CUs)."""
    assert choice_of(row, monkeypatch) == row.kernel


@pytest.mark.parametrize("walk", WALKS, ids=walk_id)
def test_the_walks_keep_their_row_s_family(walk, monkeypatch):
    row, wgs = walk
    assert choice_of(row, monkeypatch, wgs) == row.kernel


def test_every_persistent_family_is_walked_both_ways():
    for n in WALK_WGS:
        walked = {r.kernel for r, w in WALKS if w == n} | {r.kernel for r in ROWS if r.env.get("MZ_PERSIST_WGS") == str(n)}
        assert PERSISTENT <= walked, (n, sorted(PERSISTENT - walked))
