#!/usr/bin/env python3
"""Times `ultrazoom_amd.metrics.image_metrics` (PSNR + SSIM + VIF, HIP, float64) against the torch path of
`ultrazoom_amd/evaluate.py` (PSNR / ssim_per_image / vif_per_image on the same CUDA tensors) on bf16 images.

    python tools/metrics_bench.py --out profiles/metrics_bench.json

The driver never touches the GPU: every step is a child process of its own under its own time limit, and the first step that fails,
faults or runs out of time ends the run (what was measured until then is written).  Steps: the bare float64 FMA rate
(tools/microbench/mb_fma64, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing), then per shape the HIP path (all three
metrics in one call, and each metric alone) and the torch path.  Times are HIP events around `iters` calls after warm-up calls; peak memory is
torch.cuda.max_memory_allocated minus what the two images take."""

from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

SHAPES = [(1, 1080, 1920), (1, 4320, 7680), (16, 4320, 7680)]
HEADER = (REPO / "ultrazoom_amd" / "csrc" / "mz_metrics.h").read_text()
TILE_H, TILE_W, RUN = (int(re.search(rf"constexpr int {name} = (\d+);", HEADER).group(1))
                       for name in ("kMetricsTileH", "kMetricsTileW", "kMetricsRun"))  # the kernels' own constants, not copies
MB_FMA64 = REPO / "tools" / "microbench" / "mb_fma64"


def executed_fmas(B: int, H: int, W: int) -> float:
    """float64 FMAs (and the three products per staged row element) the kernels execute, whole tiles counted, from the shapes."""

    def moments(h, w, taps):
        tiles = -(-(h - taps + 1) // TILE_H) * -(-(w - taps + 1) // TILE_W)
        sh = TILE_H + taps - 1
        per_tile = sh * TILE_W * taps * 5 + sh * (TILE_W // RUN) * (taps + RUN - 1) * 3 + TILE_H * TILE_W * taps * 5
        return tiles * per_tile

    total = moments(H, W, 11)
    h, w = H, W
    for scale in range(4):
        taps = 2 ** (4 - scale) + 1
        if scale:
            h, w = (h - taps + 2) // 2, (w - taps + 2) // 2
            total += h * w * 2 * (taps * taps + taps)
        total += moments(h, w, taps)
    return float(total) * 3 * B


def images(B, H, W):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.rand((B, 3, H, W), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
    noise = torch.rand((B, 3, H, W), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
    p = (t + 0.1 * (noise - 0.5)).clamp(0, 1)
    del noise
    return p, t


def timed(fn, warmup: int, iters: int):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, torch.cuda.max_memory_allocated() - base, out


def step(kind: str, B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch

    from ultrazoom_amd.evaluate import PSNR, ssim_per_image, vif_per_image
    from ultrazoom_amd.metrics import image_metrics

    p, t = images(B, H, W)
    if kind == "hip":
        ms, peak, out = timed(lambda: image_metrics(p, t), warmup, iters)
        alone = {w: timed(lambda: image_metrics(p, t, which=(w,), data_range=1.0), 1, iters)[0] for w in ("psnr", "ssim", "vif")}
        values = {"mse": float(out["sq_err"].sum() / out["numel"].sum()), "ssim": out["ssim"].tolist(), "vif": out["vif"].tolist()}
    else:
        def torch_path():
            m = PSNR(1.0)
            m.update(p, t)
            return m, ssim_per_image(p, t), vif_per_image(p, t)

        with torch.inference_mode():
            ms, peak, out = timed(torch_path, warmup, iters)
        values = {"mse": out[0].sq / out[0].n, "ssim": out[1].tolist(), "vif": out[2].tolist()}
    image_bytes = 2 * p.numel() * p.element_size()
    fmas = executed_fmas(B, H, W)
    res = {"step": kind, "shape": [B, 3, H, W], "dtype": "bf16", "ms": ms, "warmup": warmup, "iters": iters,
           "peak_bytes_beyond_the_images": int(peak), "image_bytes": image_bytes, "values": values,
           "gbytes_per_s_two_images_read_once": image_bytes / (ms * 1e-3) / 1e9}
    if kind == "hip":
        res["executed_f64_fmas"] = fmas
        res["tfma_per_s"] = fmas / (ms * 1e-3) / 1e12
        res["ms_of_each_metric_alone"] = alone
    return res


def child(args, limit: int):
    """One step in a process of its own; None when it could not start, failed or ran out of time."""
    t0 = time.time()
    print("step:", " ".join(args[-6:]), file=sys.stderr, flush=True)
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=limit)
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
    ap.add_argument("--out", default=str(REPO / "profiles" / "metrics_bench.json"))
    ap.add_argument("--step", choices=["hip", "torch"])
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--torch-limit", type=int, default=240, help="seconds for one torch step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"fma64": None, "steps": [], "stopped": None}

    def finish(why=None):
        result["stopped"] = why
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result, indent=1))
        return 1 if why else 0

    if not MB_FMA64.exists():  # host work only: the compiler does not open the GPU
        _, err = child(["hipcc", "--offload-arch=gfx950", "-O3", str(MB_FMA64) + ".hip", "-o", str(MB_FMA64)], 300)
        if err:
            return finish(f"building mb_fma64: {err}")
    rows, err = child([str(MB_FMA64)], 120)
    if err:
        return finish(f"mb_fma64: {err}")
    result["fma64"] = rows
    torch_ms = {}
    for B, H, W in SHAPES:
        me = [sys.executable, str(Path(__file__).resolve()), "--shape", str(B), str(H), str(W)]
        rows, err = child(me + ["--step", "hip", "--warmup", str(a.warmup), "--iters", str(a.iters)], 300)
        if err:
            return finish(f"hip {B} x {H} x {W}: {err}")
        result["steps"] += rows
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")  # a file grows while the run goes on
        if B > 1:
            # sixteen times the images of the previous shape: tried only when that would fit the time limit (one call, no warm-up)
            single = torch_ms.get((1, H, W))
            if single is None or 2 * B * single * 1e-3 > a.torch_limit:
                result["steps"].append({"step": "torch", "shape": [B, 3, H, W], "ran": False,
                                        "why": f"one image took {single} ms: {B} images would not finish in {a.torch_limit} s"})
                continue
            rows, err = child(me + ["--step", "torch", "--warmup", "0", "--iters", "1"], a.torch_limit)
            if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
                result["steps"].append({"step": "torch", "shape": [B, 3, H, W], "ran": False, "why": err})
                return finish(f"torch {B} x {H} x {W}: {err}")
            result["steps"] += rows
            continue
        rows, err = child(me + ["--step", "torch", "--warmup", "1", "--iters", "2"], a.torch_limit)
        if err:
            result["steps"].append({"step": "torch", "shape": [B, 3, H, W], "ran": False, "why": err})
            return finish(f"torch {B} x {H} x {W}: {err}")
        result["steps"] += rows
        torch_ms[(B, H, W)] = rows[0]["ms"]
    return finish()


if __name__ == "__main__":
    sys.exit(main())
