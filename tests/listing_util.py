"""Device-only compiles of the kernel translation units for gfx950 (no GPU needed): resource remarks and assembly listings for the
build-time guards (tests/test_kernel_resources.py, tests/test_*_kernels.py)."""

import os
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc"
TOOLS = Path(__file__).resolve().parent.parent / "tools"
LISTINGS = {}
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def resource_usage(src: str):
    """One device-only compile per translation unit: the resource remarks on stderr, the assembly listing kept for the hazard scan."""
    asm = Path(tempfile.gettempdir()) / f"mz_guard_{os.getpid()}_{src}.s"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        str(CSRC / src), "-o", str(asm)], capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-2000:]
    LISTINGS[src] = asm
    out = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out
