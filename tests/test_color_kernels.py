"""Build-time guard on the luma unit (ultrazoom_amd/csrc/mz_color.hip): compiled for gfx950, device code only (no GPU needed).  The
streaming kernel exists once per element type and uses no LDS and no scratch; its 16-byte path is three 16-byte loads and one pinned
16-byte store; the one-plane instantiations of the metrics kernels live here (mz_metrics.hip keeps exactly the kernels it had), use no
scratch and leave room for two workgroups per CU; the listing is free of the 16-byte store-data hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage

LDS_PER_CU = 160 * 1024


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_luma_kernels_use_no_lds_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_color.hip")
    listing = LISTINGS.pop("mz_color.hip")
    try:
        for elem in range(4):
            assert sum(f"luma_kernelILi{elem}EE" in name for name in usage) == 1, (elem, sorted(usage))
            assert sum(f"luma_planes_kernelILi{elem}EE" in name for name in usage) == 1, (elem, sorted(usage))
        # the metrics of one float64 plane: PSNR, SSIM's window, the four VIF scales, the three decimations, the finish
        assert sum("psnr_kernelILi4ELi1EE" in name for name in usage) == 1, sorted(usage)
        assert sum(bool(re.search(r"moments_kernelILi4ELi\d+ELi\dELi1EE", name)) for name in usage) == 5, sorted(usage)
        assert sum("moments_kernel" in name for name in usage) == 5 and sum("down_kernel" in name for name in usage) == 3, sorted(usage)
        assert sum("finish_kernelILi1EE" in name for name in usage) == 1, sorted(usage)
        assert len(usage) == 4 + 4 + 1 + 5 + 3 + 1, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled VGPRs: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage), (sorted(lds), sorted(usage))
        for name, size in lds.items():
            if "luma_kernel" in name or "luma_planes_kernel" in name:
                assert size == 0, (name, size)
            assert 2 * size <= LDS_PER_CU, f"{name}: {size} bytes of LDS, two workgroups do not fit on a CU"
        # each streaming kernel: three 16-byte loads, and one 16-byte store, the pinned one (the store and its two wait states)
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"\n(_ZN2mz11luma_kernelILi\dEE\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)}
        assert len(bodies) == 4, sorted(bodies)
        for name, body in bodies.items():
            assert len(re.findall(r"global_load_dwordx4", body)) == 3, name
            stores = re.findall(r"(global_store_dwordx4|flat_store_dwordx4)[^\n]*\n\s*([^\n]*)", body)
            assert len(stores) == 1 and stores[0][0] == "global_store_dwordx4" and stores[0][1].strip() == "s_nop 1", (name, stores)
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
