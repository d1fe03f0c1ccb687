#!/usr/bin/env python3
"""Times the alpha kernels, in the manner of tools/ycbcr_bench.py: (a) `ultrazoom_amd.alpha_fill` and `alpha_merge` (`mz_alpha_fill`,
`mz_alpha_merge`) on 16 x 1080 x 1920 and 16 x 2160 x 3840 RGBA images, bf16 / f32 / uint8, planar ([B, 4, H, W]) and interleaved (a
permuted [B, H, W, 4] buffer), against the torch composition a user would write for the same steps on the same tensors (`avg_pool2d` for
the push, `F.interpolate(..., mode="bilinear")` for the pull, `F.interpolate(..., mode="bicubic")` for the alpha plane, tensor
expressions for the rest) and against the box's streaming rate measured in the same run; the merge enlarges the alpha plane 4 times to
the stated size and premultiplies in place.  Beside every fill: the fill of the half-size batch (what the levels from 1 up cost, nearly)
and of a 32 x 32 batch (the launches of the small levels, where time no longer follows bytes).  (b) `MewZoom.upscale_rgba` on 16 x 1080 x
1920 RGBA against `upscale_into` on the RGB part in the same run, headline model, bf16, the difference beside the budget of the added
bytes at the streaming rate.

    python tools/alpha_bench.py --out profiles/alpha_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  HIP events around every single call after
warm-up; the MEDIAN of the calls counts, the kernel and the composition timed alternately.

Algorithmic bytes, per pixel of an element size e, as mz_alpha.h moves them.  Fill: the four input elements twice (the push to level 1,
the result), three result elements, and every texel of the levels 1.. (1 / 3 of a pixel, 16 bytes) written by its push, read by the next
push, read and written by its pull, read by the finer pull: 11 e + 5 * 16 / 3.  Merge with premultiply at ratio r: the plane read
(e / r^2), the alpha written and read back (2 e), three colour elements read and written (6 e).  No threshold is set: the readings are
recorded."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from yuv_bench import HEADLINE, MB_STREAM, child, stats, timed_alternately, torch_dtype  # noqa: E402

SHAPES = ((16, 1080, 1920), (16, 2160, 3840))
WHOLE = (16, 1080, 1920)
DTYPES = ("bf16", "f32", "u8")
LAYOUTS = ("planar", "interleaved")
RATIO = 4  # of the merge


def rgba(B, H, W, dt, layout, seed=2):
    """a logical [B, 4, H, W] batch: colour noise, alpha a third zeros, a third ones, a third fractions"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (B, 4, H, W) if layout == "planar" else (B, H, W, 4)
    x = torch.empty(shape, device="cuda", dtype=torch_dtype(dt))
    v = x if layout == "planar" else x.permute(0, 3, 1, 2)
    for b in range(B):  # image by image: the float32 draw of a whole batch is large on its own
        u = torch.rand((4, H, W), device="cuda", generator=g, dtype=torch.float32)
        pick = torch.rand((1, H, W), device="cuda", generator=g, dtype=torch.float32)
        u[3:4] = torch.where(pick < 1 / 3, torch.zeros_like(pick), torch.where(pick < 2 / 3, torch.ones_like(pick), u[3:4]))
        v[b] = (u * 255 + 0.5) if dt == "u8" else u
    return v


def unit(t):
    import torch

    return t.float() / 255 if t.dtype == torch.uint8 else t.float()


def store(v, out):
    import torch

    out.copy_(v.clamp(0, 1).mul(255).add(0.5) if out.dtype == torch.uint8 else v)


def torch_fill(rgb, alpha, out):
    """the composition a user writes today: push by avg_pool2d, pull by bilinear interpolation"""
    import torch
    import torch.nn.functional as F

    a = unit(alpha).clamp(0, 1)
    c = unit(rgb)
    t = torch.where(a > 0, torch.cat([a, a * c], dim=1), torch.zeros((), device=a.device))
    pyr = [t]
    while pyr[-1].shape[2] > 1 or pyr[-1].shape[3] > 1:
        s = F.avg_pool2d(pyr[-1], 2, ceil_mode=True, divisor_override=1)
        pyr.append(s / s[:, 0:1].clamp(min=1.0))
    for l in range(len(pyr) - 2, -1, -1):
        U = F.interpolate(pyr[l + 1], size=pyr[l].shape[2:], mode="bilinear", align_corners=False)
        pyr[l] = pyr[l] + (1 - pyr[l][:, 0:1]) * U
    full = pyr[0]
    fill = (full[:, 1:] / full[:, 0:1].clamp(min=1e-30)).clamp(0, 1)
    store(torch.where(a > 0, c, fill), out)


def torch_merge(alpha, size, out):
    """bicubic alpha, clamped and stored; the colour of `out` premultiplied in place by the alpha as stored"""
    import torch.nn.functional as F

    store(F.interpolate(unit(alpha), size=size, mode="bicubic", align_corners=False).clamp(0, 1), out[:, 3:4])
    store(unit(out[:, :3]) * unit(out[:, 3:4]), out[:, :3])


def step_fill(shape, warmup, iters):
    import torch

    from ultrazoom_amd import alpha_fill

    B, H, W = shape
    rows = []
    with torch.inference_mode():
        for dt in DTYPES:
            e = torch.empty((), dtype=torch_dtype(dt)).element_size()
            for layout in LAYOUTS:
                x = rgba(B, H, W, dt, layout)
                half, small = x[:, :, : H // 2, : W // 2], x[:, :, :32, :32]
                outs = [torch.empty((B, 3, H, W), dtype=x.dtype, device="cuda") for _ in range(2)]
                hip, tor = timed_alternately([lambda: alpha_fill(x[:, :3], x[:, 3:4], out=outs[0]), lambda: torch_fill(x[:, :3], x[:, 3:4], outs[1])],
                                             warmup, iters)
                oh, os_ = outs[0][:, :, : H // 2, : W // 2], outs[0][:, :, :32, :32]
                hh, ss = timed_alternately([lambda: alpha_fill(half[:, :3], half[:, 3:4], out=oh), lambda: alpha_fill(small[:, :3], small[:, 3:4], out=os_)],
                                           warmup, iters)
                nbytes = B * H * W * (11 * e + 5 * 16 / 3)
                rows.append({"step": "fill", "dtype": dt, "layout": layout, "images": [B, H, W], "warmup": warmup, "iters": iters, "bytes": nbytes,
                             "hip": stats(hip), "torch": stats(tor), "hip_half_size": stats(hh), "hip_32x32": stats(ss),
                             "torch_over_hip": stats(tor)["median_ms"] / stats(hip)["median_ms"],
                             "hip_tbytes_per_s": nbytes / (stats(hip)["median_ms"] * 1e-3) / 1e12})
                del x, outs
                torch.cuda.empty_cache()
    return rows


def step_merge(shape, warmup, iters):
    import torch

    from ultrazoom_amd import alpha_merge

    B, H, W = shape
    h, w = H // RATIO, W // RATIO
    rows = []
    with torch.inference_mode():
        for dt in DTYPES:
            e = torch.empty((), dtype=torch_dtype(dt)).element_size()
            for layout in LAYOUTS:
                alpha = rgba(B, h, w, dt, "planar")[:, 3:4]
                outs = [rgba(B, H, W, dt, layout, seed=3 + k) for k in range(2)]
                hip, tor = timed_alternately([lambda: alpha_merge(outs[0][:, :3], alpha, size=(H, W), premultiply=True, out=outs[0]),
                                              lambda: torch_merge(alpha, (H, W), outs[1])], warmup, iters)
                nbytes = B * H * W * 8 * e + B * h * w * e
                rows.append({"step": "merge", "dtype": dt, "layout": layout, "images": [B, H, W], "from": [h, w], "mode": "bicubic", "premultiply": True,
                             "warmup": warmup, "iters": iters, "bytes": nbytes, "hip": stats(hip), "torch": stats(tor),
                             "torch_over_hip": stats(tor)["median_ms"] / stats(hip)["median_ms"],
                             "hip_tbytes_per_s": nbytes / (stats(hip)["median_ms"] * 1e-3) / 1e12})
                del alpha, outs
                torch.cuda.empty_cache()
    return rows


def step_whole(shape, warmup, iters):
    import torch

    from ultrazoom_amd import MewZoom

    B, H, W = shape
    torch.manual_seed(0)
    m = MewZoom(**HEADLINE).to("cuda", torch.bfloat16).eval()
    r = m.upscale_ratio
    with torch.inference_mode():
        x = rgba(B, H, W, "bf16", "planar")
        rgb = x[:, :3].contiguous()
        out4 = torch.empty((B, 4, r * H, r * W), dtype=torch.bfloat16, device="cuda")
        out3 = torch.empty((B, 3, r * H, r * W), dtype=torch.bfloat16, device="cuda")
        with_alpha, plain = timed_alternately([lambda: m.upscale_rgba(x, out=out4), lambda: m.upscale_into(rgb, out3)], warmup, iters)
    e = 2
    added = B * H * W * (11 * e + 5 * 16 / 3) + B * r * H * r * W * e + B * H * W * e  # the fill; the alpha plane written, its source read
    res = {"step": "whole", "model": "4X-96 (headline)", "dtype": "bf16", "images": [B, H, W], "warmup": warmup, "iters": iters, "added_bytes": added,
           "upscale_rgba": stats(with_alpha), "upscale": stats(plain)}
    res["added_ms"] = res["upscale_rgba"]["median_ms"] - res["upscale"]["median_ms"]
    return [res]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "alpha_bench.json"))
    ap.add_argument("--step", choices=("fill", "merge", "whole"))
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step:
        for row in {"fill": step_fill, "merge": step_merge, "whole": step_whole}[a.step](tuple(a.shape), a.warmup, a.iters):
            print(json.dumps(row), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "fill": [], "merge": [], "whole": None, "stopped": None}

    def finish(why=None):
        result["stopped"] = why
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps({"fill": result["fill"], "merge": result["merge"], "whole": result["whole"]}, indent=1))
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

    def run(step, shape, warmup, iters):
        rows, err = child(me + ["--step", step, "--warmup", warmup, "--iters", iters, "--shape", *shape], a.limit)
        if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
            result["steps"].append({"step": step, "shape": list(shape), "ran": False, "why": err})
            return None, f"{step} {shape}: {err}"
        result["steps"] += rows
        return rows, None

    for step in ("fill", "merge"):
        for shape in SHAPES:
            rows, err = run(step, shape, a.warmup, a.iters)
            if err:
                return finish(err)
            for got in rows:
                row = {"dtype": got["dtype"], "layout": got["layout"], "images": got["images"], "hip_ms": got["hip"]["median_ms"],
                       "torch_ms": got["torch"]["median_ms"], "torch_over_hip": got["torch_over_hip"], "bytes": got["bytes"],
                       "hip_tbytes_per_s": got["hip_tbytes_per_s"], "hip_fraction_of_stream_rate": got["hip_tbytes_per_s"] / stream}
                if step == "fill":
                    row.update(hip_half_size_ms=got["hip_half_size"]["median_ms"], hip_32x32_ms=got["hip_32x32"]["median_ms"])
                result[step].append(row)
    rows, err = run("whole", WHOLE, 1, min(a.iters, 4))
    if err:
        return finish(err)
    got = rows[0]
    result["whole"] = {"model": got["model"], "dtype": "bf16", "images": got["images"], "upscale_ms": got["upscale"]["median_ms"],
                       "upscale_rgba_ms": got["upscale_rgba"]["median_ms"], "added_ms": got["added_ms"], "added_bytes": got["added_bytes"],
                       "budget_ms_at_stream_rate": got["added_bytes"] / (stream * 1e12) * 1e3}
    return finish()


if __name__ == "__main__":
    sys.exit(main())
