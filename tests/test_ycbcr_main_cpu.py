"""The host part of ultrazoom_amd/csrc/mz_ycbcr.h under plain g++ with the address and undefined-behaviour sanitizers
(tests/ycbcr_main.cpp), in the manner of tests/test_view_checks_cpu.py: a stand-alone program, nothing of it is loaded here."""

import shutil
import subprocess
from pathlib import Path

import pytest


def test_the_header_compiles_under_plain_gxx_and_holds_under_the_sanitizers(tmp_path):
    """every 16-bit word through read and write of every depth and alignment, the constants of every matrix, range and depth (depth 8: the
    bits of yuv_coeffs), the code function at NaN and the infinities, 100 000 random (Y, Cb, Cr) triples per combination through float32
    RGB and back with zero mismatches, ycbcr_chroma_mode on strides at the ends of int64"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = Path(__file__).resolve().parent / "ycbcr_main.cpp"
    exe = tmp_path / "ycbcr_main"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ycbcr header OK" in run.stdout and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
