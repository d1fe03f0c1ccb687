"""Build-time guard on the plain-interpolation kernels (ultrazoom_amd/csrc/mz_interp.hip): compiled for gfx950, device code only (no GPU
needed), no kernel may use scratch memory or spill vector registers, there is one tile kernel per element type and mode, the LDS is what
mz_interp.h says, every 16-byte store goes through the pinned helper, and the listing is free of the 16-byte store-data hazard of
DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from interp_util import STAGE_ROWS, TILE_H, TILE_W
from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_interp_kernels_use_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_interp.hip")
    listing = LISTINGS.pop("mz_interp.hip")
    try:
        for elem in range(4):
            for mode in range(3):
                assert sum(f"interp_kernelILi{elem}ELi{mode}EE" in name for name in usage) == 1, (elem, mode, sorted(usage))
        assert len(usage) == 12, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled VGPRs: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage), lds
        for name, size in lds.items():
            elem, mode = (int(v) for v in re.search(r"interp_kernelILi(\d)ELi(\d)EE", name).groups())
            taps, chunk = (1, 2, 4)[mode], (4, 8, 8, 16)[elem]  # taps an axis; elements of a 16-byte chunk
            want = 4 * taps * (TILE_H + TILE_W) + (8 * taps * (TILE_H + TILE_W) + 8 * STAGE_ROWS * (TILE_W + chunk) if mode else 0)
            assert size == want, (name, size, want)  # indices; bilinear and bicubic: weights and the rows' (padded) horizontal sums
        assert max(lds.values()) <= 32 * 1024      # five workgroups a CU
        # every 16-byte store is the pinned one: the store and its two wait states in one statement
        stores = re.findall(r"(global_store_dwordx4|buffer_store_dwordx4|flat_store_dwordx4)[^\n]*\n\s*([^\n]*)", text)
        assert len(stores) == 12 and all(op == "global_store_dwordx4" and nxt.strip() == "s_nop 1" for op, nxt in stores), stores[:4]
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
