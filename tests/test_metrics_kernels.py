"""Build-time guard on the metrics kernels (ultrazoom_amd/csrc/mz_metrics.h): compiled for gfx950, device code only (no GPU needed),
no kernel may use scratch memory or spill vector registers, the windowed-moments kernel must leave room for two workgroups per CU, and
the listing must be free of the 16-byte store-data hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage

LDS_PER_CU = 160 * 1024


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_metrics_kernels_use_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_metrics.hip")
    listing = LISTINGS.pop("mz_metrics.hip")
    try:
        kinds = ("psnr_kernel", "psnr_reduce_kernel", "range_kernel", "moments_kernel", "down_kernel", "finish_kernel")
        for kind in kinds:
            assert any(kind in name for name in usage), f"no {kind} in the unit: {sorted(usage)}"
        # four element types for the first scale of each metric, float64 for the VIF pyramid
        assert sum("moments_kernel" in name for name in usage) == 4 + 4 + 3, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled VGPRs: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        # static LDS of every kernel, from its kernel descriptor in the listing
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", listing.read_text())}
        assert set(lds) == set(usage), (sorted(lds), sorted(usage))
        for name, size in lds.items():
            assert 2 * size <= LDS_PER_CU, f"{name}: {size} bytes of LDS, two workgroups do not fit on a CU"
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
