"""The 64-bit work-item walk of the streaming image kernels and the 32-bit walk at its limit, and the high counter word of the noise stream
(tests/far_util.py has the sizes, the data and the checks; tests/test_far_views_cpu.py holds them to non-vacuity).

luma_kernel (mz_color.hip), yuv_item (mz_yuv.hip) and yc_item (mz_ycbcr.hip) split a work item into image, row and run with 32-bit
divisions while the call has at most 2^31 - 1 items and with 64-bit divisions above.  Images one pixel wide have one run a row, so
items = B * rows: every entry runs once just inside the 32-bit branch, once at items = 2^31 exactly, H = 2^28 (the side bound), and once
with one image more ("past": at items = 2^31 every item index still fits a signed 32-bit integer, so only this size tells an `int` in the
64-bit branch from a `long long`).  Every
pixel is grey and its code is a hash of its global row: the whole of every written plane is compared on the device with a 256-entry
(depth 10: 1024-entry) table that the CPU restatements give and a small run of the same entry confirms, and blocks -- image ends, image
boundaries, the rows of items 2^31 - 1 and 2^31, random places -- are compared on the host with the restatement's float64 path.  Outputs
are pre-filled with a byte that no table entry holds; inputs are checksummed before and after.  Every comparison is an equality.

Out of scope: the 16-byte vector paths of these kernels at more than 2^31 items (16 bytes an item: 32 GiB a plane).  The item index is
taken apart before the path is chosen, so the element path exercises the same decoding.

mz_noise feeds Philox the within-image element index as two 32-bit words; one uint8 image of 2^28 x 6 pixels has 1.125 * 2^32 elements,
so the high word is 1 in the last ninth of the frame.  Blocks around element 2^32 and elsewhere are compared with degrade_ref's Philox and
Box-Muller; test_far_views_cpu.py shows that no element of these blocks lies within 1e-9 codes of a rounding tie (two float64 libraries
agree on the byte) and that the blocks past 2^32 differ from what a dropped high word would repeat.

Each case prints its wall time (fill, run, check) and its peak device memory; a case is skipped only where the device has less free
memory than its derived need."""

import gc
import time

import numpy as np
import pytest
import torch

import far_util as fu
from large_util import checksum
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

TEMPORARIES = 6 * fu.CHUNK * 8  # int64 temporaries of a chunk of hashed_codes / lut_check


@pytest.fixture(autouse=True)
def release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def need_or_skip(nbytes: int) -> None:
    assert nbytes < fu.MAX_DEVICE_BYTES, nbytes
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes / 1e9:.1f} GB of free device memory, {free / 1e9:.1f} GB are free")


def launch(name: str, B: int, H: int, codes: torch.Tensor, outs: dict, mid: torch.Tensor) -> None:
    """one call of the case's entry on [B, ., H, 1]: `codes` [B, H] is the one stored plane of the input (an RGB input reads it through a
    channel stride of 0), `mid` one chroma sample read through row and image strides of 0"""
    entry, p, _, _ = fu.WALK_CASES[name]
    plane = lambda t: (t.data_ptr(), (t.shape[1], t.shape[1], 1, 1))  # noqa: E731  a [B, rows] tensor as a [B, 1, rows, 1] view
    grey = (codes.data_ptr(), (H, 0, 1, 1))
    still = (mid.data_ptr(), (0, 0, 0, 1))
    if entry == "luma":
        _ffi.luma(*grey, *plane(outs["y"]), 3, B, H, 1, _ffi.luma_standard(p["standard"]), 0, stream())
    elif entry == "yuv420_to_rgb":
        _ffi.yuv420_to_rgb(plane(codes), still, still, (outs["rgb"].data_ptr(), (3 * H, H, 1, 1)), 3, B, H, 1,
                           *_ffi.yuv_codes(p["matrix"], p["range_"], p["siting"]), 1, stream())
    elif entry == "rgb_to_yuv420":
        _ffi.rgb_to_yuv420(grey, 3, plane(outs["y"]), plane(outs["cb"]), plane(outs["cr"]), B, H, 1,
                           *_ffi.yuv_codes(p["matrix"], p["range_"], p["siting"]), stream())
    else:
        fmt, codes3 = _ffi.ycbcr_codes(p["depth"], p["align"], p["sub"], p["matrix"], p["range_"], p["siting"])
        if entry == "ycbcr_to_rgb":
            _ffi.ycbcr_to_rgb(plane(codes), still, still, *fmt, (outs["rgb"].data_ptr(), (3 * H, H, 1, 1)), 3, B, H, 1, *codes3, 1, stream())
        else:
            _ffi.rgb_to_ycbcr(grey, 3, plane(outs["y"]), plane(outs["cb"]), plane(outs["cr"]), *fmt, B, H, 1, *codes3, stream())
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def tables():
    """name -> (tables, sentinel), each confirmed by a small run of the entry over all codes (one image, one code a row)"""
    out = {}
    for name in fu.WALK_CASES:
        luts = fu.walk_luts(name)
        sentinel = fu.walk_sentinel(name, luts)
        n = next(iter(luts.values())).numel() if "cb" not in luts else luts["y"].numel()
        codes = torch.arange(n, dtype=torch.int64, device="cuda").to(fu.walk_src_dtype(name)).view(1, n)
        mid = torch.full((8,), fu.walk_mid(name), dtype=fu.walk_src_dtype(name), device="cuda")
        outs = fu.walk_outputs(name, 1, n, "cuda", sentinel)
        launch(name, 1, n, codes, outs, mid)
        for k, plane in fu.walk_planes(outs).items():
            want = luts[k].expand(plane.shape[1]) if k in ("cb", "cr") else luts[k]
            assert torch.equal(plane[0].cpu(), want), f"{name}: a run over all {n} codes does not give the table of plane '{k}'"
        out[name] = (luts, sentinel)
    return out


@pytest.mark.parametrize("name, branch", fu.WALK_RUNS, ids=lambda v: str(v))
def test_long_walk(name, branch, tables):
    B, H, per = fu.walk_shape(name, branch)
    entry, _, lo, hi = fu.WALK_CASES[name]
    items = fu.walk_items(entry, branch)
    assert items == {32: (1 << 31) - B, 64: 1 << 31, "past": (1 << 31) + (1 << 28)}[branch], items
    luts, sentinel = tables[name]
    src = fu.walk_src_dtype(name)
    es = torch.empty((), dtype=src).element_size()
    rows_out = {"luma": 1, "yuv420_to_rgb": 3, "ycbcr_to_rgb": 3, "rgb_to_yuv420": 2, "rgb_to_ycbcr": 3}[entry]
    need_or_skip(B * H * (es + rows_out) + TEMPORARIES)
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    codes = fu.hashed_codes(B, H, "cuda", lo, hi, dtype=src)
    mid = torch.full((8,), fu.walk_mid(name), dtype=src, device="cuda")
    outs = fu.walk_outputs(name, B, H, "cuda", sentinel)
    before = checksum(codes), checksum(mid)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    launch(name, B, H, codes, outs, mid)
    t2 = time.perf_counter()
    assert (checksum(codes), checksum(mid)) == before, f"{name}: the run changed its input"
    blocks = fu.walk_verify(name, B, H, per, codes, outs, luts, sentinel)
    t3 = time.perf_counter()
    peak = torch.cuda.max_memory_allocated()
    print(f"long walk {name}, branch {branch}: B = {B}, H = {H}, {items} items; fill {t1 - t0:.2f} s, run {t2 - t1:.2f} s, check {t3 - t2:.2f} s "
          f"({blocks} blocks), peak device memory {peak / 1e9:.2f} GB")
    assert peak < fu.MAX_DEVICE_BYTES


def test_noise_counter_high_word():
    H, W, n = fu.NOISE_H, fu.NOISE_W, fu.NOISE_BLOCK
    total = 3 * H * W
    assert total > 1 << 32
    need_or_skip(total + (1 << 28))
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    x = torch.empty((1, 3, H, W), dtype=torch.uint8, device="cuda")
    for c in range(3):  # (no call spans 2^31 elements)
        x[0, c].fill_(fu.NOISE_FILL)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _ffi.noise(x.data_ptr(), x.stride(), x.data_ptr(), x.stride(), 3, 1, H, W, fu.NOISE_SIGMA, fu.NOISE_SEED, 0, stream())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    flat = x.view(-1)
    blocks = fu.noise_blocks()
    for label, first in blocks:
        want, sure = fu.noise_expected(first)
        assert bool(sure.all()), f"block '{label}': the reference has an element on a rounding tie"
        got = flat[first : first + n].cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"noise block '{label}' (elements {first}..): {bad.size} of {n} bytes differ from the checker; first at element "
                               f"{first + int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}")
        if first >= 1 << 32:
            low, _ = fu.noise_expected(first, high_word=False)
            assert int((low != want).sum()) > n // 2, f"block '{label}': a dropped high word would give the same bytes"
    t3 = time.perf_counter()
    peak = torch.cuda.max_memory_allocated()
    print(f"noise {H} x {W} uint8, {total} elements: fill {t1 - t0:.2f} s, run {t2 - t1:.2f} s, check {t3 - t2:.2f} s ({len(blocks)} blocks), "
          f"peak device memory {peak / 1e9:.2f} GB")
    assert peak < fu.MAX_DEVICE_BYTES
