"""Build-time guard on the degradation kernels (ultrazoom_amd/csrc/mz_degrade.h): compiled for gfx950, device code only (no GPU needed),
no kernel may use scratch memory or spill vector registers (the blur weights and the quantisation tables travel as kernel arguments and
are indexed there: an argument copied to private memory would show as scratch), there is one kernel of each family per element type,
the static LDS of a workgroup stays under 32 KiB (two workgroups and more per CU), and the listing is free of the 16-byte store-data
hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage

FAMILIES = ("blur_kernelILi", "noise_kernelILi", "jpeg_code_kernelILi", "jpeg_image_kernelILi")


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_degrade_kernels_use_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_degrade.hip")
    listing = LISTINGS.pop("mz_degrade.hip")
    try:
        for family in FAMILIES:
            assert sum(family in name for name in usage) == 4, (family, sorted(usage))
        assert len(usage) == 16, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled VGPRs: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", listing.read_text())}
        assert set(lds) == set(usage), lds
        for name, size in lds.items():
            assert size <= 32 * 1024, (name, size)
            assert (size > 0) == ("blur_kernel" in name or "jpeg_code_kernel" in name), (name, size)
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)


def test_the_blur_tile_and_its_halo_fit_the_static_arrays():
    header = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_degrade.h").read_text()
    half, tile = (int(re.search(rf"constexpr int {n} = (\d+);", header).group(1)) for n in ("kBlurMaxHalf", "kBlurTile"))
    assert (half, tile) == (15, 32) and tile + 2 * half <= 64  # the staged tile's row pitch is 64 floats
