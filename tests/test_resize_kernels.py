"""Build-time guard on the resampling kernels (ultrazoom_amd/csrc/mz_resize.h): compiled for gfx950, device code only (no GPU needed), no
kernel may use scratch memory or spill vector registers, there is one resize_kernel per element type, none holds static LDS (the
dynamic LDS is sized per call: at most 43 KiB at the ratio-16 limit), and the listing is free of the 16-byte store-data hazard of
DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_resize_kernels_use_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_resize.hip")
    listing = LISTINGS.pop("mz_resize.hip")
    try:
        assert sum("resize_table_kernel" in name for name in usage) == 1, sorted(usage)
        assert sum("resize_kernelILi" in name for name in usage) == 4, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled VGPRs: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", listing.read_text())}
        assert set(lds) == set(usage) and not any(lds.values()), lds
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)


def test_the_largest_lds_request_fits_one_allocation():
    """resize_plan()'s figures at the ratio-16 limit, restated: 66 taps, 7 * 16 + 1 + 66 rows of 32 float32, double weights."""
    header = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_resize.h").read_text()
    th, tw, taps, ratio = (int(re.search(rf"constexpr int {n} = (\d+);", header).group(1))
                           for n in ("kResizeTileH", "kResizeTileW", "kResizeMaxTaps", "kResizeMaxRatio"))
    rows = (th - 1) * ratio + 1 + taps
    assert (taps * tw + taps * th) * 8 + rows * tw * 4 <= 64 * 1024
