"""Every conv and mix family on data that make its arithmetic exact (tests/exact_util.py): the output must equal the float64 result
rounded once to the storage type, bit for bit -- fp32 accumulation, ONE nearest-even rounding, z rounded before the gate and the blend.
No tolerance and no sibling kernel; only the elements whose gate (or SiLU) argument lies inside (SAT_LO, SAT_HI), where the
transcendental is not exact, are compared with the one-operator tolerance instead.  tests/test_exact_cpu.py holds the data to the
conditions that keep these equalities from being vacuous."""

import pytest

from exact_util import ROWS, WALKS, exact, row_id, walk_id
from op_util import check_rounded_once, launch, set_knobs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_bit_for_bit(row, monkeypatch):
    set_knobs(monkeypatch, row.env)
    ex = exact(row)
    out, got = launch(row.entry, row.args, row.dt, ex.inputs, ex.alpha)
    check_rounded_once(row, row_id(row), ex, out, got)


@pytest.mark.parametrize("walk", WALKS, ids=walk_id)
def test_bit_for_bit_persistent_walks(walk, monkeypatch):
    """The same row with 8 and with 16 persistent workgroups: each run equals the expectation, not merely the other run."""
    row, wgs = walk
    set_knobs(monkeypatch, row.env, wgs)
    ex = exact(row)
    out, got = launch(row.entry, row.args, row.dt, ex.inputs, ex.alpha)
    check_rounded_once(row, row_id(row), ex, out, got)
