"""Repository rules that keep the parity claims honest."""

import re
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_product_package_never_touches_the_oracle_or_the_reference():
    for path in (REPO / "ultrazoom_amd").rglob("*"):
        if path.suffix not in {".py", ".cpp", ".hip", ".h", ".sh"}:
            continue
        text = path.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f"{path} imports the oracle"
        assert "/root/reference" not in text, f"{path} reads the reference at run time"
        if path.name == "evaluate.py":
            # the PSNR / SSIM harness measures images that were ALREADY upscaled (its Gaussian window is a torch
            # convolution); it is not on the upscale path and must not carry any of the model's arithmetic
            assert "def upscale" not in text and "def forward" not in text
            continue
        assert "torch.nn.functional" not in text and "F.conv2d" not in text, f"{path} has a PyTorch compute path"


def test_gpu_side_files_do_not_read_the_reference():
    for rel in ("bench.py", "__graft_entry__.py"):
        p = REPO / rel
        if p.exists():
            assert "/root/reference" not in p.read_text()
    for p in (REPO / "tests").glob("test_*.py"):
        if p.name == "test_layout.py":
            continue
        assert "/root/reference" not in p.read_text(), p


def test_no_file_under_tests_imports_a_test_module():
    """What test modules share lives in a *_util.py / *_ref.py / op_cases.py: a CPU test never stands on a GPU test file, and a kernel
    family is registered in a table, not in a test (conftest is no test module)."""
    for p in sorted((REPO / "tests").rglob("*.py")):
        found = re.findall(r"^\s*(?:from|import)\s+test_\w+.*", p.read_text(), re.M)
        assert not found, f"{p} imports from a test module: {found}"


def test_no_struct_name_is_defined_in_two_image_headers():
    """The image headers (mz_view.h and those that include it) put their structs into namespace mz of one shared object: two definitions
    of one name are one type to the linker (undefined behaviour where they differ), whichever translation units see them."""
    seen = {}
    for p in sorted((REPO / "ultrazoom_amd" / "csrc").glob("*.h")):
        text = p.read_text()
        if p.name != "mz_view.h" and '#include "mz_view.h"' not in text:
            continue
        for name in re.findall(r"^struct\s+(\w+)\s*\{", text, re.M):  # (column 0: namespace scope)
            assert name not in seen, f"struct {name} is defined in {seen[name]} and in {p.name}"
            seen[name] = p.name
    assert {"StridedView", "MetricsFinishArgs", "EnsembleFinishArgs", "InterpArgs", "ResizeArgs", "DegradeArgs", "Refusal"} <= set(seen)


def test_the_knob_list_is_what_read_knobs_reads():
    """op_util.set_knobs clears op_cases.KNOBS: a knob read_knobs() (mz_plan.h) reads and the list does not name would leak from the
    environment into every test that pins a kernel."""
    from op_cases import KNOBS
    from op_util import knob_names

    assert len(KNOBS) == len(set(KNOBS)) and set(KNOBS) == knob_names(), (sorted(KNOBS), sorted(knob_names()))
