#!/usr/bin/env python3
"""Are the kernels of the working tree the SAME MACHINE CODE as those of another commit?

    tools/cmp_listings.py [--base REV] [--work DIR] [--jobs N] [--rename OLD=NEW ..] [unit ...]
                                                                      (units: mz_conv3r mz_conv3t ..; default: every csrc/*.hip)

Compiles every unit device-only to a gfx950 assembly listing -- the flags of tests/test_kernel_resources.py, no GPU needed -- once from
`git archive REV` (default HEAD; kept in DIR/<commit> and reused) and once from the working tree, and compares the listings PER KERNEL
SYMBOL after removing what differs between any two compiles of equal code: the __hip_cuid_* symbol, a function's ordinal in its
.LBB<n>_<m> / .Lfunc_end<n> labels and loop comments, the .file / .ident lines.  What lies outside the functions (the code-object
metadata: argument layouts, register counts) is compared as the pseudo symbol <module>.  Prints a count per unit; exit status 1 if
anything differs, and then DIR/diff/<unit>.<n>.diff holds the first differing symbols.

--rename OLD=NEW (repeatable) substitutes text in the base listing before it is split into symbols: a struct a kernel takes by value is
part of the kernel's mangled name, so renaming the struct (say 10ResizeView=11StridedView) would otherwise report every kernel as
"only in base".

For refactors of kernels that live at their register cap, where "about as fast" is not a criterion one can check without a GPU and
"the same listing" is.
"""
import argparse
import difflib
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = "ultrazoom_amd/csrc"
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"]

NORMALISE = [
    (re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_#"),
    (re.compile(r"\bBB\d+_(\d+)"), r"BB#_\1"),
    (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1#"),
]
DROP = re.compile(r"^\s*\.(file|ident)\b")
BEGIN = re.compile(r"; -- Begin function (\S+)")
TAIL = re.compile(r"^\s*\.section\s+\.AMDGPU\.gpr_maximums|__hip_cuid_")


def symbols(listing: Path, renames=()):
    """{symbol: normalised lines}; '<module>' = everything in front of the first and behind the last function."""
    out = {"<module>": []}
    cur = "<module>"
    text = listing.read_text()
    for old, new in renames:
        text = text.replace(old, new)
    for line in text.splitlines():
        if DROP.match(line):
            continue
        m = BEGIN.search(line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur != "<module>" and TAIL.search(line):
            cur = "<module>"
        for pat, to in NORMALISE:
            line = pat.sub(to, line)
        out[cur].append(line)
    return out


def compile_unit(src_dir: Path, unit: str, out_dir: Path):
    out_dir.mkdir(parents=True, exist_ok=True)
    out = out_dir / f"{unit}.s"
    p = subprocess.run([HIPCC, *FLAGS, str(src_dir / f"{unit}.hip"), "-o", str(out)], capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"{unit} ({src_dir}): hipcc failed\n{p.stderr[-3000:]}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("units", nargs="*")
    ap.add_argument("--base", default="HEAD", help="commit to compare the working tree against")
    ap.add_argument("--work", default=str(Path(tempfile.gettempdir()) / "mz_cmp_listings"), help="where listings are kept")
    ap.add_argument("--jobs", type=int, default=4, help="hipcc processes side by side")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="text substitution in the base listing")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    work = Path(args.work)
    units = args.units or sorted(p.stem for p in (ROOT / CSRC).glob("*.hip"))
    sha = subprocess.run(["git", "-C", str(ROOT), "rev-parse", args.base], capture_output=True, text=True, check=True).stdout.strip()
    base_dir = work / sha
    if not (base_dir / "src").exists():
        (base_dir / "src").mkdir(parents=True)
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", sha, CSRC], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", str(base_dir / "src")], input=tar, check=True)
    jobs = [(base_dir / "src" / CSRC, u, base_dir / "s") for u in units if not (base_dir / "s" / f"{u}.s").exists()]
    jobs += [(ROOT / CSRC, u, work / "head") for u in units]
    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))

    bad = 0
    for u in units:
        b, h = symbols(base_dir / "s" / f"{u}.s", renames), symbols(work / "head" / f"{u}.s")
        differing = [s for s in sorted(set(b) | set(h)) if b.get(s) != h.get(s)]
        every = set(b) | set(h)
        print(f"{u}: {len(every) - len(differing)} of {len(every)} symbols identical (<module> + {len(every) - 1} functions)")
        for n, s in enumerate(differing):
            bad += 1
            what = "only in base" if s not in h else "only in head" if s not in b else "differs"
            print(f"    {what}: {s}")
            if n < 4 and s in b and s in h:
                (work / "diff").mkdir(exist_ok=True)
                d = work / "diff" / f"{u}.{n}.diff"
                d.write_text("\n".join(difflib.unified_diff(b[s], h[s], "base " + s, "head " + s, lineterm="", n=4)) + "\n")
                print(f"        {d}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
