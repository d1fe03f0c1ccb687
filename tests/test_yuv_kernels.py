"""Build-time guard on the 4:2:0 YCbCr unit (ultrazoom_amd/csrc/mz_yuv.hip), in the manner of tests/test_color_kernels.py: compiled for
gfx950, device code only (no GPU needed).  One kernel per RGB element type and direction and nothing else; no scratch, no spilled
registers, no LDS (two workgroups fit on a CU with room to spare); every 16-byte store is the pinned one of mz_view.h; the listing is free
of the 16-byte store-data hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage

LDS_PER_CU = 160 * 1024
KERNELS = ("yuv420_to_rgb_kernel", "rgb_to_yuv420_kernel")


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_yuv_kernels_use_no_lds_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_yuv.hip")
    listing = LISTINGS.pop("mz_yuv.hip")
    try:
        for kernel in KERNELS:
            for elem in range(4):
                assert sum(f"{kernel}ILi{elem}EE" in name for name in usage) == 1, (kernel, elem, sorted(usage))
        assert len(usage) == 8, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0 or v.get("SGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled registers: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage), (sorted(lds), sorted(usage))
        for name, size in lds.items():
            assert 2 * size <= LDS_PER_CU, f"{name}: {size} bytes of LDS, two workgroups do not fit on a CU"
            assert size == 0, (name, size)
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"\n(_ZN2mz\d+\w+_kernelILi\dEE\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)}
        assert len(bodies) == 8, sorted(bodies)
        for name, body in bodies.items():
            assert "flat_store_dwordx4" not in body and "flat_load_dwordx4" not in body, name
            stores = re.findall(r"global_store_dwordx4[^\n]*\n\s*([^\n]*)", body)
            assert stores and all(s.strip() == "s_nop 1" for s in stores), (name, stores)  # the store and its two wait states: store16
            assert "global_load_dwordx4" in body, name
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
