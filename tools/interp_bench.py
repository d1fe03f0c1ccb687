#!/usr/bin/env python3
"""Times the plain-interpolation kernel (`mz_interpolate`, bicubic x4) against torch's own `F.interpolate(mode="bicubic")` on the same dense
CUDA tensors in the same run -- what a user would otherwise call for the model's bicubic baseline.

    python tools/interp_bench.py --out profiles/interp_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  Steps: the box's streaming rate
(tools/microbench/mb_stream, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing; the best variant counts), then per
element type (bf16, u8) 16 x 1080x1920 -> 4320x7680: the kernel on its separable path, the kernel forced down its gather path
(MZ_INTERP_GATHER), and torch (bf16 only: torch has no uint8 bicubic on the device; there the comparison is the chain a user writes,
`.float() / 255 -> interpolate -> clamp -> * 255 + 0.5 -> uint8`, image by image to bound its float32 intermediates).  HIP events around
every single call after warm-up; the MEDIAN of the calls counts.  Algorithmic bytes: every input element read once, every output element
written once (bf16: 3.4 GB).

Acceptance (margin 1.0, the same run, the same tensors): the kernel is not slower than torch.  The fraction of the stream rate is
recorded, not promised."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

SHAPE = (16, 1080, 1920)
RATIO = 4
DTYPES = ("bf16", "u8")
MB_STREAM = REPO / "tools" / "microbench" / "mb_stream"


def image(B, H, W, dt):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    if dt == "u8":
        x = torch.empty((B, 3, H, W), device="cuda", dtype=torch.uint8)
        for b in range(B):
            x[b].random_(0, 256, generator=g)
        return x
    return torch.rand((B, 3, H, W), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)


def timed(fn, warmup: int, iters: int):
    """the time of every single call, by device events"""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in events:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in events]


def step(kind: str, dt: str, B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch
    import torch.nn.functional as F

    from ultrazoom_amd.interpolate import interpolate

    x = image(B, H, W, dt)
    out = torch.empty((B, 3, RATIO * H, RATIO * W), dtype=x.dtype, device="cuda")
    if kind == "torch" and dt == "u8":
        def fn():
            for b in range(B):
                y = F.interpolate(x[b:b + 1].float().div_(255), scale_factor=RATIO, mode="bicubic", align_corners=False)
                out[b:b + 1] = y.clamp_(0, 1).mul_(255).add_(0.5).to(torch.uint8)
    elif kind == "torch":
        def fn():
            out.copy_(F.interpolate(x, scale_factor=RATIO, mode="bicubic", align_corners=False).clamp_(0, 1))
    else:
        if kind == "gather":
            os.environ["MZ_INTERP_GATHER"] = "1"
        fn = lambda: interpolate(x, scale_factor=RATIO, mode="bicubic", clamp=True, out=out)  # noqa: E731
    with torch.inference_mode():
        ms = timed(fn, warmup, iters)
    nbytes = x.element_size() * (x.numel() + out.numel())
    med = statistics.median(ms)
    return {"step": kind, "dtype": dt, "shape": [B, 3, H, W], "ratio": RATIO, "warmup": warmup, "iters": iters, "median_ms": med, "min_ms": min(ms),
            "max_ms": max(ms), "bytes": nbytes, "tbytes_per_s": nbytes / (med * 1e-3) / 1e12, "checksum": float(out[0, :, ::16, ::16].float().mean())}


def child(args, limit: int):
    """One step in a process of its own under `timeout -k 10`; None when it could not start, failed or ran out of time."""
    t0 = time.time()
    print("step:", " ".join(str(a) for a in args[-10:]), file=sys.stderr, flush=True)
    try:
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + [str(a) for a in args], capture_output=True, text=True, timeout=limit + 30)
    except subprocess.TimeoutExpired:
        return None, f"no result within {limit} s"
    except OSError as e:
        return None, f"could not start: {e}"
    if r.returncode != 0:
        return None, f"exit status {r.returncode} after {time.time() - t0:.0f} s: {r.stderr.strip()[-400:]}"
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            rows.append(json.loads(line))
        elif line.startswith("["):
            rows += json.loads(line)
    print(f"  {time.time() - t0:.0f} s:", json.dumps(rows)[:600], file=sys.stderr, flush=True)
    return rows, None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "interp_bench.json"))
    ap.add_argument("--step", choices=["hip", "gather", "torch"])
    ap.add_argument("--dtype", choices=DTYPES)
    ap.add_argument("--shape", type=int, nargs=3, default=list(SHAPE))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "summary": [], "acceptance": None, "stopped": None}

    def write():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")

    def finish(why=None):
        result["stopped"] = why
        write()
        print(json.dumps({"summary": result["summary"], "acceptance": result["acceptance"]}, indent=1))
        if why:
            print("stopped:", why)
        return 1 if why else 0

    if not MB_STREAM.exists():  # host work only: the compiler does not open the GPU
        _, err = child(["hipcc", "--offload-arch=gfx950", "-O3", str(MB_STREAM) + ".hip", "-o", str(MB_STREAM)], 300)
        if err:
            return finish(f"building mb_stream: {err}")
    rows, err = child([str(MB_STREAM)], 120)
    if err:
        return finish(f"mb_stream: {err}")
    result["stream"] = rows
    result["stream_tbytes_per_s"] = stream = max(r["TB_per_s"] for r in rows)
    me = [sys.executable, str(Path(__file__).resolve()), "--warmup", a.warmup, "--iters", a.iters, "--shape", *a.shape]
    worst = None
    for dt in DTYPES:
        got = {}
        for kind in ("hip", "gather", "torch"):
            rows, err = child(me + ["--step", kind, "--dtype", dt], a.limit)
            if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
                result["steps"].append({"step": kind, "dtype": dt, "ran": False, "why": err})
                return finish(f"{kind} {dt}: {err}")
            result["steps"] += rows
            got[kind] = rows[0]
            write()  # the file grows while the run goes on
        ratio = got["torch"]["median_ms"] / got["hip"]["median_ms"]
        worst = ratio if worst is None else min(worst, ratio)
        result["summary"].append({
            "dtype": dt, "shape": got["hip"]["shape"], "hip_ms": got["hip"]["median_ms"], "gather_ms": got["gather"]["median_ms"],
            "torch_ms": got["torch"]["median_ms"], "torch_over_hip": ratio, "hip_tbytes_per_s": got["hip"]["tbytes_per_s"],
            "hip_fraction_of_stream_rate": got["hip"]["tbytes_per_s"] / stream,
            "torch_fraction_of_stream_rate": got["torch"]["tbytes_per_s"] / stream,
        })
    result["acceptance"] = {"worst_torch_over_hip": worst, "not_slower_than_torch": worst >= 1.0}
    return finish()


if __name__ == "__main__":
    sys.exit(main())
