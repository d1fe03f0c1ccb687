#!/usr/bin/env python3
"""Times `ultrazoom_amd.resize.resize` (antialiased bicubic, HIP) against torch's own antialiased `interpolate` on the same CUDA
tensors, bf16 and uint8.

    python tools/resize_bench.py --out profiles/resize_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  Steps: the box's streaming rate
(tools/microbench/mb_stream, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing; the best variant counts, as
profiles/r03_mb_stream.json records them), then per shape and element type the HIP kernel and the torch path.  Times are HIP events
around `iters` calls after warm-up calls.  Algorithmic bytes = the input elements the outputs need (all of them at these ratios) plus
the output elements, each moved once.  Where torch has no kernel for an element type the step says so and float32 is timed instead."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

# (B, Hin, Win, Hout, Wout)
SHAPES = [(1, 1080, 1920, 540, 960), (1, 4320, 7680, 2160, 3840), (16, 4320, 7680, 2160, 3840), (16, 4320, 7680, 3240, 5760)]
DTYPES = ("bf16", "u8")
MB_STREAM = REPO / "tools" / "microbench" / "mb_stream"


def image(B, H, W, dt):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    if dt == "u8":
        return torch.randint(0, 256, (B, 3, H, W), device="cuda", generator=g, dtype=torch.uint8)
    x = torch.empty((B, 3, H, W), device="cuda", dtype=torch.bfloat16)
    for b in range(B):  # image by image: no float32 copy of the whole batch
        x[b] = torch.rand((3, H, W), device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
    return x


def timed(fn, warmup: int, iters: int):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def step(kind: str, dt: str, B: int, H: int, W: int, Ho: int, Wo: int, warmup: int, iters: int) -> dict:
    import torch
    import torch.nn.functional as F

    from ultrazoom_amd.resize import resize

    x = image(B, H, W, dt)
    res = {"step": kind, "dtype": dt, "shape": [B, 3, H, W], "size": [Ho, Wo], "warmup": warmup, "iters": iters}
    if kind == "hip":
        out = torch.empty((B, 3, Ho, Wo), dtype=x.dtype, device="cuda")
        ms, out = timed(lambda: resize(x, (Ho, Wo), out=out), warmup, iters)
        res["checksum"] = float(out.float().mean())
    else:
        def torch_path(v):
            return F.interpolate(v, size=(Ho, Wo), mode="bicubic", antialias=True, align_corners=False)

        with torch.inference_mode():
            try:
                torch_path(x[:1, :, :64, :64])
                torch.cuda.synchronize()
                src = x
            except RuntimeError as e:  # no kernel of this element type in torch's HIP build: float32 stands in, and the row says so
                res["torch_dtype"] = "float32"
                res["why_float32"] = str(e).splitlines()[0][:200]
                src = None
            if src is None:
                src = torch.empty((B, 3, H, W), device="cuda", dtype=torch.float32)
                for b in range(B):
                    src[b] = x[b].float() / (255.0 if dt == "u8" else 1.0)
            ms, out = timed(lambda: torch_path(src), warmup, iters)
        res["checksum"] = float(out.float().mean()) / (255.0 if out.dtype == torch.uint8 else 1.0)
    nbytes = (x.numel() + B * 3 * Ho * Wo) * x.element_size()
    res.update(ms=ms, algorithmic_bytes=nbytes, algorithmic_tbytes_per_s=nbytes / (ms * 1e-3) / 1e12)
    return res


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
    ap.add_argument("--out", default=str(REPO / "profiles" / "resize_bench.json"))
    ap.add_argument("--step", choices=["hip", "torch"])
    ap.add_argument("--dtype", choices=DTYPES)
    ap.add_argument("--shape", type=int, nargs=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "summary": [], "stopped": None}

    def write():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")

    def finish(why=None):
        result["stopped"] = why
        write()
        print(json.dumps(result["summary"], indent=1))
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
    for B, H, W, Ho, Wo in SHAPES:
        for dt in DTYPES:
            me = [sys.executable, str(Path(__file__).resolve()), "--dtype", dt, "--shape", B, H, W, Ho, Wo, "--warmup", a.warmup, "--iters", a.iters]
            pair = {}
            for kind in ("hip", "torch"):
                rows, err = child(me + ["--step", kind], a.limit)
                if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
                    result["steps"].append({"step": kind, "dtype": dt, "shape": [B, 3, H, W], "size": [Ho, Wo], "ran": False, "why": err})
                    return finish(f"{kind} {dt} {B} x {H} x {W} -> {Ho} x {Wo}: {err}")
                result["steps"] += rows
                pair[kind] = rows[0]
                write()  # the file grows while the run goes on
            result["summary"].append({
                "dtype": dt, "shape": [B, 3, H, W], "size": [Ho, Wo], "hip_ms": pair["hip"]["ms"], "torch_ms": pair["torch"]["ms"],
                "torch_dtype": pair["torch"].get("torch_dtype", dt), "torch_over_hip": pair["torch"]["ms"] / pair["hip"]["ms"],
                "algorithmic_tbytes_per_s": pair["hip"]["algorithmic_tbytes_per_s"],
                "fraction_of_stream_rate": pair["hip"]["algorithmic_tbytes_per_s"] / stream,
            })
    return finish()


if __name__ == "__main__":
    sys.exit(main())
