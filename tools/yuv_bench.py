#!/usr/bin/env python3
"""Times the 4:2:0 YCbCr kernels, in the manner of tools/color_bench.py: (a) `ultrazoom_amd.yuv420_to_rgb` and `rgb_to_yuv420`
(`mz_yuv420_to_rgb`, `mz_rgb_to_yuv420`) on 16 frames of 2160 x 3840 inside NV12 and I420 frame buffers, RGB as bf16, f32 and uint8,
against the torch composition a user would write for the same conversion -- `F.interpolate(..., mode="bilinear")` for the chroma of
"center" siting, the matrix as tensor expressions, `avg_pool2d` for the way back -- on the same tensors in the same process, and against
the box's streaming rate; (b) `MewZoom.upscale_yuv420` on 16 NV12 frames of 1080 x 1920 against `upscale` on the equivalent RGB batch,
headline model, bf16.

    python tools/yuv_bench.py --out profiles/yuv_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  Steps: the box's streaming rate
(tools/microbench/mb_stream, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing; the best variant counts), then one
step per direction, layout and RGB type -- the kernel and the composition timed alternately, call by call -- then (b).  HIP events around
every single call after warm-up; the MEDIAN of the calls counts.  Algorithmic bytes of (a): every plane byte and every RGB element
moved once, 1.5 + 3 * (bytes of an RGB element) per pixel.

CONDITION: no case of (a) is slower than the composition (`torch_over_hip` >= 1.0); `condition_holds` records it and the exit status
follows it.  The fractions of the streaming rate are recorded, not fixed in advance.  The budget of (b)'s added time is three times the
conversions' bytes (7.5 per input pixel and 7.5 per output pixel) at the measured streaming rate."""

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

FRAMES = (16, 2160, 3840)
WHOLE = (16, 1080, 1920)
DTYPES = ("bf16", "f32", "u8")
LAYOUTS = ("nv12", "i420")
DIRECTIONS = ("to_rgb", "to_yuv")
PARAMS = dict(matrix="bt709", range="limited", siting="center")  # "center": the siting F.interpolate and avg_pool2d compute
KR, KB, YOFF, SY, SC = 0.2126, 0.0722, 16.0, 219.0, 224.0
MB_STREAM = REPO / "tools" / "microbench" / "mb_stream"
HEADLINE = dict(upscale_ratio=4, primary_channels=96, primary_layers=8, secondary_channels=192, secondary_layers=8, tertiary_channels=384,
                tertiary_layers=8, quaternary_channels=768, quaternary_layers=16, hidden_ratio=2, num_deg_features=3)


def torch_dtype(dt):
    import torch

    return {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}[dt]


def frames(B, H, W, seed=1):
    """a [B, H * 3 / 2, W] uint8 frame buffer of random codes"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.empty((B, H * 3 // 2, W), device="cuda", dtype=torch.uint8)
    for b in range(B):
        buf[b].random_(0, 256, generator=g)
    return buf


def cut(buf, layout):
    from ultrazoom_amd import i420_planes, nv12_planes

    return nv12_planes(buf) if layout == "nv12" else i420_planes(buf)


def rgb_image(B, H, W, dt, seed=2):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((B, 3, H, W), device="cuda", dtype=torch_dtype(dt))
    for b in range(B):  # image by image: the float32 draw of a whole batch is large on its own
        if dt == "u8":
            x[b].random_(0, 256, generator=g)
        else:
            x[b] = torch.rand((3, H, W), device="cuda", generator=g, dtype=torch.float32)
    return x


def torch_to_rgb(y, cb, cr, out):
    """the composition a user writes today: bilinear chroma, the matrix as tensor expressions, the store rule of the dtype"""
    import torch
    import torch.nn.functional as F

    kg = 1.0 - KR - KB
    yn = (y.float() - YOFF) / SY
    cbn, crn = ((F.interpolate(c.float(), scale_factor=2, mode="bilinear", align_corners=False) - 128.0) / SC for c in (cb, cr))
    rgb = torch.cat([yn + 2 * (1 - KR) * crn, yn - (2 * KR * (1 - KR) / kg) * crn - (2 * KB * (1 - KB) / kg) * cbn, yn + 2 * (1 - KB) * cbn], dim=1)
    rgb = rgb.clamp_(0, 1)
    out.copy_(rgb.mul_(255).add_(0.5) if out.dtype == torch.uint8 else rgb)


def torch_to_yuv(x, y, cb, cr):
    import torch
    import torch.nn.functional as F

    v = x.float() / 255 if x.dtype == torch.uint8 else x.float()
    r, g, b = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    lum = KR * r + (1.0 - KR - KB) * g + KB * b
    y.copy_((lum * SY + YOFF).clamp_(0, 255).add_(0.5))
    cb.copy_((F.avg_pool2d((b - lum) * (0.5 / (1 - KB)), 2) * SC + 128.0).clamp_(0, 255).add_(0.5))
    cr.copy_((F.avg_pool2d((r - lum) * (0.5 / (1 - KR)), 2) * SC + 128.0).clamp_(0, 255).add_(0.5))


def timed_alternately(fns, warmup: int, iters: int):
    """the time of every single call of each function, by device events; the functions take turns"""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(iters)]
    for turn in events:
        for fn, (e0, e1) in zip(fns, turn):
            e0.record()
            fn()
            e1.record()
    torch.cuda.synchronize()
    return [[turn[i][0].elapsed_time(turn[i][1]) for turn in events] for i in range(len(fns))]


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step_convert(direction: str, layout: str, dt: str, B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch

    from ultrazoom_amd import rgb_to_yuv420, yuv420_to_rgb

    elem = torch.empty((), dtype=torch_dtype(dt)).element_size()
    nbytes = B * H * W * 3 // 2 + B * 3 * H * W * elem
    res = {"step": direction, "layout": layout, "dtype": dt, "frames": [B, H, W], "warmup": warmup, "iters": iters, "bytes": nbytes, **PARAMS}
    with torch.inference_mode():
        if direction == "to_rgb":
            planes = cut(frames(B, H, W), layout)
            out_hip, out_torch = (torch.empty((B, 3, H, W), dtype=torch_dtype(dt), device="cuda") for _ in range(2))
            hip, tor = timed_alternately([lambda: yuv420_to_rgb(*planes, out=out_hip, **PARAMS), lambda: torch_to_rgb(*planes, out_torch)], warmup, iters)
            diff = (out_hip[0, :, ::8, ::8].float() - out_torch[0, :, ::8, ::8].float()).abs().max()
            res["max_abs_difference_sampled"] = float(diff) / (255.0 if dt == "u8" else 1.0)
        else:
            x = rgb_image(B, H, W, dt)
            buf_hip, buf_torch = (torch.zeros((B, H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(2))
            p_hip, p_torch = cut(buf_hip, layout), cut(buf_torch, layout)
            hip, tor = timed_alternately([lambda: rgb_to_yuv420(x, out=p_hip, **PARAMS), lambda: torch_to_yuv(x, *p_torch)], warmup, iters)
            res["max_code_difference_sampled"] = int((buf_hip[0, ::4, ::4].int() - buf_torch[0, ::4, ::4].int()).abs().max())
    res["hip"], res["torch"] = stats(hip), stats(tor)
    res["hip_tbytes_per_s"] = nbytes / (res["hip"]["median_ms"] * 1e-3) / 1e12
    res["torch_over_hip"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
    return res


def step_whole(B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch

    from ultrazoom_amd import MewZoom, nv12_planes, yuv420_to_rgb

    torch.manual_seed(0)
    m = MewZoom(**HEADLINE).to("cuda", torch.bfloat16).eval()
    r = m.upscale_ratio
    with torch.inference_mode():
        src = nv12_planes(frames(B, H, W))
        dst = nv12_planes(torch.zeros((B, r * H * 3 // 2, r * W), dtype=torch.uint8, device="cuda"))
        kw = dict(matrix="bt709", range="limited", siting="left")
        rgb = yuv420_to_rgb(*src, dtype=torch.bfloat16, **kw)  # the equivalent RGB batch
        out = torch.empty((B, 3, r * H, r * W), dtype=torch.bfloat16, device="cuda")
        yuv, plain = timed_alternately([lambda: m.upscale_yuv420(*src, out=dst, **kw), lambda: m.upscale_into(rgb, out)], warmup, iters)
    res = {"step": "whole", "model": "4X-96 (headline)", "dtype": "bf16", "layout": "nv12", "frames": [B, H, W], "warmup": warmup, "iters": iters,
           "upscale_yuv420": stats(yuv), "upscale": stats(plain)}
    res["added_ms"] = res["upscale_yuv420"]["median_ms"] - res["upscale"]["median_ms"]
    res["conversion_bytes"] = int(7.5 * B * H * W + 7.5 * B * r * H * r * W)
    res["checksum"] = float(dst[0][0, 0, ::16, ::16].float().mean())
    return res


def child(args, limit: int):
    """One step in a process of its own under `timeout -k 10`; None when it could not start, failed or ran out of time."""
    t0 = time.time()
    print("step:", " ".join(str(a) for a in args[-12:]), file=sys.stderr, flush=True)
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
    ap.add_argument("--out", default=str(REPO / "profiles" / "yuv_bench.json"))
    ap.add_argument("--step", choices=DIRECTIONS + ("whole",))
    ap.add_argument("--layout", choices=LAYOUTS)
    ap.add_argument("--dtype", choices=DTYPES)
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step == "whole":
        print(json.dumps(step_whole(*a.shape, a.warmup, a.iters)), flush=True)
        return 0
    if a.step:
        print(json.dumps(step_convert(a.step, a.layout, a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "convert": [], "whole": None, "condition_holds": None, "stopped": None}

    def write():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")

    def finish(why=None):
        result["stopped"] = why
        if not why:
            result["condition_holds"] = all(c["torch_over_hip"] >= 1.0 for c in result["convert"])
        write()
        print(json.dumps({"convert": result["convert"], "whole": result["whole"], "condition_holds": result["condition_holds"]}, indent=1))
        if why:
            print("stopped:", why)
        return 0 if not why and result["condition_holds"] else 1

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

    def run(args, shape, warmup, iters):
        rows, err = child(me + ["--warmup", warmup, "--iters", iters, "--shape", *shape] + args, a.limit)
        if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
            result["steps"].append({"args": args, "ran": False, "why": err})
            return None, f"{' '.join(args)}: {err}"
        result["steps"] += rows
        write()  # the file grows while the run goes on
        return rows[0], None

    for direction in DIRECTIONS:
        for layout in LAYOUTS:
            for dt in DTYPES:
                got, err = run(["--step", direction, "--layout", layout, "--dtype", dt], FRAMES, a.warmup, a.iters)
                if err:
                    return finish(err)
                result["convert"].append({"direction": direction, "layout": layout, "dtype": dt, "frames": got["frames"],
                                          "hip_ms": got["hip"]["median_ms"], "torch_ms": got["torch"]["median_ms"],
                                          "torch_over_hip": got["torch_over_hip"], "hip_tbytes_per_s": got["hip_tbytes_per_s"],
                                          "hip_fraction_of_stream_rate": got["hip_tbytes_per_s"] / stream})
    got, err = run(["--step", "whole"], WHOLE, 1, min(a.iters, 4))
    if err:
        return finish(err)
    budget_ms = 3.0 * got["conversion_bytes"] / (stream * 1e12) * 1e3
    result["whole"] = {"model": got["model"], "dtype": "bf16", "layout": "nv12", "frames": got["frames"],
                       "upscale_ms": got["upscale"]["median_ms"], "upscale_yuv420_ms": got["upscale_yuv420"]["median_ms"],
                       "added_ms": got["added_ms"], "conversion_bytes": got["conversion_bytes"], "budget_ms": budget_ms,
                       "within_budget": got["added_ms"] <= budget_ms}
    return finish()


if __name__ == "__main__":
    sys.exit(main())
