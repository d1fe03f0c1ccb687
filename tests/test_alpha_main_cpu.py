"""The host part of ultrazoom_amd/csrc/mz_alpha.h under plain g++ with the address and undefined-behaviour sanitizers
(tests/alpha_main.cpp), in the manner of tests/test_ycbcr_main_cpu.py: a stand-alone program, nothing of it is loaded here."""

import shutil
import subprocess
from pathlib import Path

import pytest


def test_the_header_compiles_under_plain_gxx_and_holds_under_the_sanitizers(tmp_path):
    """the level sizes and the workspace at the ends of int and of the accepted range; one texel through level 0, push and pull at NaN,
    infinities and the ends of float32; the neighbour rule at sides of 2^28; the exact-constant property of one push and pull"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = Path(__file__).resolve().parent / "alpha_main.cpp"
    exe = tmp_path / "alpha_main"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "alpha header OK" in run.stdout and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
