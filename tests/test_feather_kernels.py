"""Build-time guard on the feather unit (ultrazoom_amd/csrc/mz_feather.hip), in the manner of tests/test_alpha_kernels.py: compiled for
gfx950, device code only (no GPU needed).  Exactly the four instantiations of feather_paste_kernel; no scratch, no spilled registers, no
LDS, no atomics; every 16-byte store is the pinned one of mz_view.h and every 16-byte load a global one; the listing is free of the
16-byte store-data hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_feather_kernels_are_the_expected_ones_without_scratch_spills_lds_or_store_hazard():
    usage = resource_usage("mz_feather.hip")
    listing = LISTINGS.pop("mz_feather.hip")
    try:
        for elem in range(4):
            assert sum(f"feather_paste_kernelILi{elem}EE" in name for name in usage) == 1, (elem, sorted(usage))
        assert len(usage) == 4, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0 or v.get("SGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled registers: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        print({k: (v.get("VGPRs"), v.get("SGPRs"), v.get("Occupancy")) for k, v in usage.items()})
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage) and all(size == 0 for size in lds.values()), lds
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"\n(_ZN2mz\d+feather_paste_kernel\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)}
        assert set(bodies) == set(usage), (sorted(bodies), sorted(usage))
        for name, body in bodies.items():
            assert "flat_store_dwordx4" not in body and "flat_load_dwordx4" not in body and "scratch_" not in body, name
            assert "atomic" not in body and "ds_" not in body, name
            stores = re.findall(r"global_store_dwordx4[^\n]*\n\s*([^\n]*)", body)
            assert stores and all(s.strip() == "s_nop 1" for s in stores), (name, stores)  # the store and its two wait states: store16
            assert "global_load_dwordx4" in body, name
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
