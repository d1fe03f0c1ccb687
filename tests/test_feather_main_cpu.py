"""The host part of ultrazoom_amd/csrc/mz_feather.h under plain g++ with the address and undefined-behaviour sanitizers
(tests/feather_main.cpp), in the manner of tests/test_alpha_main_cpu.py: a stand-alone program, nothing of it is loaded here."""

import shutil
import subprocess
from pathlib import Path

import pytest


def test_the_header_compiles_under_plain_gxx_and_holds_under_the_sanitizers(tmp_path):
    """omega(n, n - 1) < 1 and growing weights for every ramp up to 2^20; the ramp bounds at the ends of int; the blend and the uint8
    code at their extremes"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = Path(__file__).resolve().parent / "feather_main.cpp"
    exe = tmp_path / "feather_main"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "feather header OK" in run.stdout and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
