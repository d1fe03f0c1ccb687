"""Build-time guard on the dihedral / ensemble kernels (ultrazoom_amd/csrc/mz_dihedral.hip): compiled for gfx950, device code only (no
GPU needed), no kernel may use scratch memory or spill vector registers, there is one tile skeleton per element type and mode and one
finish kernel per element type, the tile's LDS is the one static [64][65] dword image, every 16-byte store goes through the pinned
helper, and the listing is free of the 16-byte store-data hazard of DESIGN.md section 4.1."""

import re
import sys
from pathlib import Path

import pytest

from listing_util import HIPCC, LISTINGS, TOOLS, resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_dihedral_kernels_use_no_scratch_and_have_no_store_hazard():
    usage = resource_usage("mz_dihedral.hip")
    listing = LISTINGS.pop("mz_dihedral.hip")
    try:
        assert sum("dihedral_kernelILi" in name for name in usage) == 8, sorted(usage)       # 4 element types x {copy, accumulate}
        assert sum("ensemble_finish_kernelILi" in name for name in usage) == 4, sorted(usage)
        bad = {k: v for k, v in usage.items() if v.get("ScratchSize", 0) != 0 or v.get("VGPRs Spill", 0) != 0}
        assert not bad, "kernels with scratch memory / spilled VGPRs: " + ", ".join(f"{k}: {v}" for k, v in bad.items())
        text = listing.read_text()
        lds = {m.group(1): int(m.group(2))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)}
        assert set(lds) == set(usage), lds
        for name, size in lds.items():
            assert size == (64 * 65 * 4 if "dihedral_kernel" in name else 0), (name, size)
        # every 16-byte store is the pinned one: the store and its two wait states in one statement
        stores = re.findall(r"(global_store_dwordx4|buffer_store_dwordx4|flat_store_dwordx4)[^\n]*\n\s*([^\n]*)", text)
        assert stores and all(op == "global_store_dwordx4" and nxt.strip() == "s_nop 1" for op, nxt in stores), stores[:4]
        assert "global_load_dwordx4" in text  # the 16-byte path exists on the load side too
        sys.path.insert(0, str(TOOLS))
        import asm_store_hazard

        assert asm_store_hazard.scan(str(listing)) == 0
    finally:
        listing.unlink(missing_ok=True)


def test_the_lds_pitch_is_conflict_free_for_rows_and_columns():
    """The bank arithmetic of mz_dihedral.h, restated: dword (r, c) of the tile lies on bank (r * pitch + c) % 32.  32 lanes along a row
    and 32 lanes along a column both cover every bank once; with the 16-byte paths (a lane owns 4 / 8 / 16 consecutive dwords) a bank is
    shared by two lanes of a group at the most.  A pitch of 64 would put a column on ONE bank."""
    header = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_dihedral.h").read_text()
    tile = int(re.search(r"constexpr int kDihedralTile = (\d+);", header).group(1))
    pitch = tile + 1

    def worst(lanes):  # lanes: the (r, c) of one 32-lane group
        banks = [(r * pitch + c) % 32 for r, c in lanes]
        return max(banks.count(b) for b in set(banks))

    for start in (0, 32):
        assert worst([(7, start + l) for l in range(32)]) == 1       # along a row
        assert worst([(start + l, 7) for l in range(32)]) == 1       # along a column
    assert len({(r * 64 + 7) % 32 for r in range(32)}) == 1
    for vec in (4, 8, 16):
        per_row = tile // vec
        for e in range(vec):
            # the load side writes row-major chunks; the store side of a transposing orientation reads the same chunks column-major
            lanes = [(l // per_row, (l % per_row) * vec + e) for l in range(32)]
            assert worst(lanes) <= 2, (vec, e)
            assert worst([(c, r) for r, c in lanes]) <= 2, (vec, e)
