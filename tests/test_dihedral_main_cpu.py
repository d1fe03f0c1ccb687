"""ultrazoom_amd/csrc/mz_dihedral.h -- the one statement of the eight orientations, which the device kernels and the host entries
compile -- as a stand-alone host program under the sanitizers (tests/dihedral_main.cpp)."""

import shutil
import subprocess
from pathlib import Path

import pytest


def test_the_transform_header_walks_every_orientation_under_the_sanitizers(tmp_path):
    """Every k over the shapes 1 x 1 .. 5 x 7: source index, output shape and inverse against a restatement by whole-table flips and a
    transposition, built from the HIP-free header alone with the address and undefined-behaviour sanitizers (an index outside the image
    ends it).  A stand-alone host program: nothing of it is loaded here."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = Path(__file__).resolve().parent / "dihedral_main.cpp"
    exe = tmp_path / "dihedral_main"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "dihedral checks OK" in run.stdout and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
