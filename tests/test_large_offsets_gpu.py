"""Every 32-bit-offset kernel family up to its guard, and its fallback one row past it (tests/large_util.py has the table and the method).

Per case: inputs filled on the device with seeded integers, the output pre-filled with NaN, ONE run of the entry; then the family that ran,
a 64-bit checksum of every input before and after, the WHOLE output on the device -- no NaN (a dropped store leaves one), everything
finite, and bit for bit equal to fp32 matmuls rounded once; the channel counts of the table are all multiples of 16, so none of these
cases HAS pad channels and the sweep's pad-channel count checks nothing here -- and blocks at the corners, at the pixels where an offset
crosses 2^31 / 2^32 and at random places against float64 on the host.  Every comparison is an equality, or gpu_util's one-operator
tolerance for the elements inside the transcendental's window (at most MAX_EXCLUDED of a case) and for the head's bicubic skip.  An
out-of-range buffer load returns zeros and an out-of-range buffer store is dropped: nothing here would fault, it would be wrong."""

import gc
import time

import pytest
import torch

import large_util as lu
from exact_util import MAX_EXCLUDED
from gpu_util import DTYPES, alloc_act, last_kernel
from op_util import run_entry, set_knobs

pytestmark = pytest.mark.gpu

# peak of torch's allocator (the case's tensors and the sweep's temporaries).  What the library allocates itself per call -- weight
# packings, a tile list, the zero page: megabytes -- and the caching allocator's slack (printed as "reserved") are not in this figure.
MAX_DEVICE_BYTES = 20e9


@pytest.fixture(autouse=True)
def release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", lu.CASES, ids=lambda c: c.name)
def test_large_offsets(case, monkeypatch):
    set_knobs(monkeypatch)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    started = time.perf_counter()
    dtype = DTYPES[case.dt]
    t = lu.make_inputs(case, "cuda", alloc_act=alloc_act)
    C, shape = lu.out_shape(case)
    out = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    sums = {k: lu.checksum(v) for k, v in t.items()}

    run_entry(case.entry, lu.op_args(case), case.dt, t, out)
    if case.kernel is not None:
        assert last_kernel() == case.kernel, (last_kernel(), case.kernel)
    for k, v in t.items():
        assert lu.checksum(v) == sums[k], f"{case.name}: the run changed its input '{k}'"

    if case.entry == "final":  # the bicubic skip is not exact: the whole tensor for NaN, blocks for values
        rep = lu.Report()
        lu.whole_tensor_counts(out, 512, rep)
        assert rep.nan == 0 and rep.nonfinite == 0, f"{case.name}: {rep.nan} NaN, {rep.nonfinite} non-finite elements in the output"
    else:
        rep = lu.sweep(case, t, out)
        print(f"{case.name}: swept {rep.total} elements, excluded share {rep.excluded:.5f} ({rep.soft} elements), sums {rep.sums}")
        lu.assert_report(case, rep, MAX_EXCLUDED)
        assert rep.total + rep.soft == case.B * C * shape[2] * shape[3]
    swept = time.perf_counter()
    blocks = lu.pick_blocks(case)
    for blk in blocks:
        lu.check_block(case, t, out, blk)
    peak = torch.cuda.max_memory_allocated()
    done = time.perf_counter()
    print(f"{case.name}: {last_kernel() if case.kernel else '-'}, peak device memory {peak / 1e9:.2f} GB (reserved {torch.cuda.max_memory_reserved() / 1e9:.2f}), {done - started:.2f} s "
          f"(fill + run + sweep {swept - started:.2f} s, {len(blocks)} blocks {done - swept:.2f} s), excluded {rep.excluded:.5f} "
          f"(worst {rep.soft_excess:.2f} x the one-operator tolerance, fp32 bound {rep.sums.get('soft_bound', 0.0):.2f} x)")
    assert peak < MAX_DEVICE_BYTES
