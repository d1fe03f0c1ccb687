#!/usr/bin/env python3
"""Times the luma kernels: (a) `ultrazoom_amd.rgb_to_y` (`mz_luma`) against the torch expression a user would write for the same plane,
`(x.float() * k.view(1, 3, 1, 1)).sum(1) + off`, on the same dense CUDA tensors in the same run, and against the box's streaming rate;
(b) `image_metrics(luma="bt601")` (`mz_metrics_luma`: one plane of metric work) against the RGB call on the same pair.

    python tools/color_bench.py --out profiles/color_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  Steps: the box's streaming rate
(tools/microbench/mb_stream, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing; the best variant counts), then
(a) per element type (bf16, f32, u8) 16 x 4320x7680: the kernel, then torch; then (b) 16 x 2160x3840 bf16: the luma metrics, then the
RGB metrics.  HIP events around every single call after warm-up; the MEDIAN of the calls counts.  Algorithmic bytes of (a): every input
element read once, every output element written once.

No threshold is fixed: the readings and the two ratios (torch over kernel; RGB metrics over luma metrics) are recorded."""

from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

LUMA_SHAPE = (16, 4320, 7680)
METRICS_SHAPE = (16, 2160, 3840)
DTYPES = ("bf16", "f32", "u8")
MB_STREAM = REPO / "tools" / "microbench" / "mb_stream"


def image(B, H, W, dt, seed=1):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    if dt == "u8":
        x = torch.empty((B, 3, H, W), device="cuda", dtype=torch.uint8)
        for b in range(B):
            x[b].random_(0, 256, generator=g)
        return x
    x = torch.empty((B, 3, H, W), device="cuda", dtype={"bf16": torch.bfloat16, "f32": torch.float32}[dt])
    for b in range(B):  # image by image: the float32 draw of a whole 16 x 8K batch is 6 GB on its own
        x[b] = torch.rand((3, H, W), device="cuda", generator=g, dtype=torch.float32)
    return x


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


def row(kind, dt, shape, warmup, iters, ms, **more):
    med = statistics.median(ms)
    return {"step": kind, "dtype": dt, "shape": [shape[0], 3, shape[1], shape[2]], "warmup": warmup, "iters": iters, "median_ms": med,
            "min_ms": min(ms), "max_ms": max(ms), **more}


def step(kind: str, dt: str, B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch

    from ultrazoom_amd import rgb_to_y
    from ultrazoom_amd.evaluate import LUMA_COEFFS
    from ultrazoom_amd.metrics import image_metrics

    with torch.inference_mode():
        if kind in ("luma_hip", "luma_torch"):
            x = image(B, H, W, dt)
            nbytes = x.element_size() * (x.numel() + x.numel() // 3)
            if kind == "luma_hip":
                out = torch.empty((B, 1, H, W), dtype=x.dtype, device="cuda")
                ms = timed(lambda: rgb_to_y(x, "bt601", out=out), warmup, iters)
                check = float(out[0, 0, ::16, ::16].float().mean())
            else:
                off, k = LUMA_COEFFS["bt601"][0], torch.tensor(LUMA_COEFFS["bt601"][1:], device="cuda", dtype=torch.float32)
                keep = []

                def fn():
                    keep[:] = [(x.float() * k.view(1, 3, 1, 1)).sum(1) + off]

                ms = timed(fn, warmup, iters)
                check = float(keep[0][0, ::16, ::16].mean())
            med = statistics.median(ms)
            return row(kind, dt, (B, H, W), warmup, iters, ms, bytes=nbytes, tbytes_per_s=nbytes / (med * 1e-3) / 1e12, checksum=check)
        p, t = image(B, H, W, dt, 1), image(B, H, W, dt, 2)
        luma = "bt601" if kind == "metrics_luma" else None
        res = {}

        def fn():
            res.update(image_metrics(p, t, luma=luma))

        ms = timed(fn, warmup, iters)
        alone = {w: statistics.median(timed(lambda: image_metrics(p, t, which=(w,), data_range=1.0, luma=luma), 1, iters)) for w in ("psnr", "ssim", "vif")}
        return row(kind, dt, (B, H, W), warmup, iters, ms, ms_of_each_metric_alone=alone,
                   values={"mse": float(res["sq_err"].sum() / res["numel"].sum()), "ssim": float(res["ssim"].mean()), "vif": float(res["vif"].mean())})


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
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    print(f"  {time.time() - t0:.0f} s:", json.dumps(rows)[:600], file=sys.stderr, flush=True)
    return rows, None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "color_bench.json"))
    ap.add_argument("--step", choices=["luma_hip", "luma_torch", "metrics_luma", "metrics_rgb"])
    ap.add_argument("--dtype", choices=DTYPES)
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "luma": [], "metrics": None, "stopped": None}

    def write():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")

    def finish(why=None):
        result["stopped"] = why
        write()
        print(json.dumps({"luma": result["luma"], "metrics": result["metrics"]}, indent=1))
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
    me = [sys.executable, str(Path(__file__).resolve())]

    def run(kind, dt, shape, warmup, iters):
        rows, err = child(me + ["--warmup", warmup, "--iters", iters, "--shape", *shape, "--step", kind, "--dtype", dt], a.limit)
        if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
            result["steps"].append({"step": kind, "dtype": dt, "ran": False, "why": err})
            return None, f"{kind} {dt}: {err}"
        result["steps"] += rows
        write()  # the file grows while the run goes on
        return rows[0], None

    for dt in DTYPES:
        got = {}
        for kind in ("luma_hip", "luma_torch"):
            got[kind], err = run(kind, dt, LUMA_SHAPE, a.warmup, a.iters)
            if err:
                return finish(err)
        hip, tor = got["luma_hip"], got["luma_torch"]
        result["luma"].append({"dtype": dt, "shape": hip["shape"], "hip_ms": hip["median_ms"], "torch_ms": tor["median_ms"],
                               "torch_over_hip": tor["median_ms"] / hip["median_ms"], "hip_tbytes_per_s": hip["tbytes_per_s"],
                               "hip_fraction_of_stream_rate": hip["tbytes_per_s"] / stream})
    got = {}
    for kind in ("metrics_luma", "metrics_rgb"):
        got[kind], err = run(kind, "bf16", METRICS_SHAPE, 2, min(a.iters, 5))
        if err:
            return finish(err)
    result["metrics"] = {"dtype": "bf16", "shape": got["metrics_rgb"]["shape"], "luma_ms": got["metrics_luma"]["median_ms"],
                         "rgb_ms": got["metrics_rgb"]["median_ms"], "rgb_over_luma": got["metrics_rgb"]["median_ms"] / got["metrics_luma"]["median_ms"]}
    return finish()


if __name__ == "__main__":
    sys.exit(main())
