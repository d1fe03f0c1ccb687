"""Build-time guard on the YCbCr unit of any depth and subsampling (ultrazoom_amd/csrc/mz_ycbcr.hip), in the manner of
tests/test_yuv_kernels.py: compiled for gfx950, device code only (no GPU needed).  One kernel per RGB element type, sample type and
direction and nothing else; no scratch, no spilled registers, no LDS; every 16-byte store is the pinned one of mz_view.h; the listing is
free of the 16-byte store-data hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage

KERNELS = ("ycbcr_to_rgb_kernel", "rgb_to_ycbcr_kernel")


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_ycbcr_kernels_use_no_lds_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_ycbcr.hip")
    listing = LISTINGS.pop("mz_ycbcr.hip")
    try:
        for kernel in KERNELS:
            for elem in range(4):
                for sample in range(2):
                    assert sum(f"{kernel}ILi{elem}ELi{sample}EE" in name for name in usage) == 1, (kernel, elem, sample, sorted(usage))
        assert len(usage) == 16, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0 or v.get("SGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled registers: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage), (sorted(lds), sorted(usage))
        assert all(size == 0 for size in lds.values()), lds
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"\n(_ZN2mz\d+\w+_kernelILi\dELi\dEE\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)}
        assert len(bodies) == 16, sorted(bodies)
        for name, body in bodies.items():
            assert "flat_store_dwordx4" not in body and "flat_load_dwordx4" not in body and "scratch_" not in body, name
            stores = re.findall(r"global_store_dwordx4[^\n]*\n\s*([^\n]*)", body)
            assert stores and all(s.strip() == "s_nop 1" for s in stores), (name, stores)  # the store and its two wait states: store16
            assert "global_load_dwordx4" in body, name
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
