"""Build-time guard on the alpha unit (ultrazoom_amd/csrc/mz_alpha.hip), in the manner of tests/test_ycbcr_kernels.py: compiled for
gfx950, device code only (no GPU needed).  The expected instantiations and nothing else; no scratch, no spilled registers; LDS in the
merge kernel only (the taps of a tile); every 16-byte store is the pinned one of mz_view.h; the listing is free of the 16-byte store-data
hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage

PER_ELEM = ("alpha_push0_kernel", "alpha_pull0_kernel", "alpha_premultiply_kernel")  # <E>
PLAIN = ("alpha_push_kernel", "alpha_pull_kernel")                                   # texels only
MERGE_LDS = {0: 4 * (128 + 32), 1: 2 * (4 + 8) * (128 + 32), 2: 4 * (4 + 8) * (128 + 32)}  # the taps: int indices, double weights


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_alpha_kernels_are_the_expected_ones_without_scratch_spills_or_store_hazard():
    usage = resource_usage("mz_alpha.hip")
    listing = LISTINGS.pop("mz_alpha.hip")
    try:
        for kernel in PER_ELEM:
            for elem in range(4):
                assert sum(f"{kernel}ILi{elem}EE" in name for name in usage) == 1, (kernel, elem, sorted(usage))
        for kernel in PLAIN:
            assert sum(re.search(rf"\d+{kernel}E", name) is not None for name in usage) == 1, (kernel, sorted(usage))
        for elem in range(4):
            for mode in range(3):
                assert sum(f"alpha_merge_kernelILi{elem}ELi{mode}EE" in name for name in usage) == 1, (elem, mode, sorted(usage))
        assert len(usage) == 3 * 4 + 2 + 12, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0 or v.get("SGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled registers: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage), (sorted(lds), sorted(usage))
        for name, size in lds.items():
            m = re.search(r"alpha_merge_kernelILi\dELi(\d)EE", name)
            assert size == (MERGE_LDS[int(m.group(1))] if m else 0), (name, size)
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"\n(_ZN2mz\d+alpha_\w+_kernel\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)}
        assert set(bodies) == set(usage), (sorted(bodies), sorted(usage))
        for name, body in bodies.items():
            assert "flat_store_dwordx4" not in body and "flat_load_dwordx4" not in body and "scratch_" not in body, name
            assert "atomic" not in body, name
            stores = re.findall(r"global_store_dwordx4[^\n]*\n\s*([^\n]*)", body)
            assert stores and all(s.strip() == "s_nop 1" for s in stores), (name, stores)  # the store and its two wait states: store16
            if "alpha_merge_kernel" not in name:  # (the merge gathers single elements of the small plane)
                assert "global_load_dwordx4" in body, name
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)
