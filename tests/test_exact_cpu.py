"""The exact-arithmetic table (tests/exact_util.py) held to the conditions that keep tests/test_exact_gpu.py from being vacuous, with
the float64 reference alone: no GPU.  These are conditions on the test data, not measurements of a kernel."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from exact_util import (CENSUS_MIN, CENSUS_MIN_SHARE, EXACT_SUM, F16_MAX_OUT, MAX_EXCLUDED, MIN_BRANCH, PERSISTENT, ROWS, WALK_WGS, WALKS, bits_of, census, exact, lower_edge, round_once, row_id,
                        walk_id)
from gpu_util import DTYPES
from test_poison_ops_gpu import FAMILY_OF_UNREPORTED, KNOBS, SELECT_OP
from ultrazoom_amd import _ffi


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
    src = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_select.h").read_text()
    body = re.search(r"inline const char\* kernel_name\(const KernelChoice& ch\) \{(.*?)\n\}\n", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = set(re.findall(r'"([a-z0-9_]+)"', body))
    assert len(names) >= 15 and {"conv3r", "conv3t_fused", "mix16b", "conv_kernel_mix"} <= names, names
    covered = {r.kernel for r in ROWS if r.kernel} | {FAMILY_OF_UNREPORTED[r.entry] for r in ROWS if r.entry in FAMILY_OF_UNREPORTED}
    assert names <= covered, f"no row runs {sorted(names - covered)}"
    assert PERSISTENT <= names
    assert len({row_id(r) for r in ROWS}) == len(ROWS)
    # every dtype of every family ending in _mix or _fused, and both 16-bit mix kernels
    gated = {n for n in names if n.endswith(("_mix", "_fused"))} | {"mix16", "mix16b"}
    assert gated <= {r.kernel for r in ROWS if r.entry in ("mix", "conv_mix")}


def selected(row, monkeypatch, wgs=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    if wgs is not None:
        monkeypatch.setenv("MZ_PERSIST_WGS", str(wgs))
    lib = _ffi.lib()
    lib.mz_debug_select.restype = ctypes.c_char_p
    B, H, W = row.args[:3]
    if row.entry == "mix":
        op, cin, cout = 7, 2 * row.args[3], row.args[3]
    elif row.entry == "final":
        op, cin, cout = 3, row.args[3], 12
    else:
        cin, cout = row.args[3:5]
        op = SELECT_OP[row.entry] if row.entry != "conv" else (0 if row.silu else 1)
    got = lib.mz_debug_select(_ffi.dtype_code(DTYPES[row.dt]), op, cin, cout, B, H, W, 256)
    return got.decode() if got is not None else None


@pytest.mark.parametrize("row", [r for r in ROWS if r.entry in SELECT_OP], ids=row_id)
def test_the_pinned_families_are_the_host_s_choice(row, monkeypatch):
    """With SiLU off, and for this table's own shapes: the name of every row is what the host chooses on an MI355X (256 CUs)."""
    assert selected(row, monkeypatch) == row.kernel


@pytest.mark.parametrize("walk", WALKS, ids=walk_id)
def test_the_walks_keep_their_row_s_family(walk, monkeypatch):
    row, wgs = walk
    assert selected(row, monkeypatch, wgs) == row.kernel


def test_every_persistent_family_is_walked_both_ways():
    for n in WALK_WGS:
        walked = {r.kernel for r, w in WALKS if w == n} | {r.kernel for r in ROWS if r.env.get("MZ_PERSIST_WGS") == str(n)}
        assert PERSISTENT <= walked, (n, sorted(PERSISTENT - walked))
