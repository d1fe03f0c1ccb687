#!/usr/bin/env python3
"""Times feathered tiling, in the manner of tools/alpha_bench.py: (a) `ultrazoom_amd.feather_paste` (`mz_feather_paste`) alone on 16 x
2160 x 3840 images, bf16 / f32 / uint8, with no ramp, a ramp of 128 columns and a ramp of 128 rows, against the torch composition a user
would write on the same tensors (`dst.copy_(src)` outside the band, `torch.lerp` with a weight tensor inside it) and against the box's
streaming rate measured in the same run; (b) the headline model in bf16 on one 2160 x 3840 image: `upscale_tiled(tile=1024)` (exact,
halo = the receptive field) against `upscale_feathered(tile=1024, halo=32)` and `upscale_feathered(tile=512, halo=32)`, alternated, the
measured ratios beside the ones `tiling.tile_work` predicts, and the summed time of the pastes of one run; (c) the deviation of
`upscale_feathered` from `upscale` on 1 x 1080 x 1920 for halo 8 .. 128 with overlap = halo // 2, blended and hard-cut (overlap 0):
max-abs and PSNR.  (b) and (c) run on SYNTHETIC weights (the seeded default initialisation): they say nothing about trained checkpoints.

    python tools/feather_bench.py --out profiles/feather_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  HIP events around every single call after
warm-up; the MEDIAN of the calls counts, the compared versions timed alternately.

Algorithmic bytes of a paste of N elements of size e of which R lie under a ramp: two reads and one write inside the ramps, one read
and one write outside -- e (3 R + 2 (N - R)).  No threshold is set: the readings are recorded."""

from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from yuv_bench import HEADLINE, MB_STREAM, child, rgb_image, stats, timed_alternately, torch_dtype  # noqa: E402

PASTE = (16, 2160, 3840)
WHOLE = (1, 2160, 3840)
DEVIATION = (1, 1080, 1920)
DTYPES = ("bf16", "f32", "u8")
RAMPS = ((0, 0), (0, 128), (128, 0))
HALOS = (8, 16, 32, 64, 128)


def torch_paste(src, dst, ramp, weight):
    """the composition a user writes today: a copy outside the band, a lerp with a weight tensor inside it"""
    import torch

    ny, nx = ramp
    if not ny and not nx:
        dst.copy_(src)
        return
    band, rest = ((..., slice(0, ny), slice(None)), (..., slice(ny, None), slice(None))) if ny else ((..., slice(0, nx)), (..., slice(nx, None)))
    dst[rest].copy_(src[rest])
    d, s = dst[band], src[band]
    if dst.dtype == torch.uint8:
        d.copy_(torch.lerp(d.float(), s.float(), weight).add_(0.5))
    else:
        d.copy_(torch.lerp(d, s, weight))


def step_paste(shape, warmup, iters):
    import torch

    from ultrazoom_amd import feather_paste

    B, H, W = shape
    rows = []
    with torch.inference_mode():
        for dt in DTYPES:
            e = torch.empty((), dtype=torch_dtype(dt)).element_size()
            src = rgb_image(B, H, W, dt, seed=2)
            dsts = [rgb_image(B, H, W, dt, seed=3) for _ in range(2)]
            for ny, nx in RAMPS:
                n = ny or nx
                w = (2 * torch.arange(n, device="cuda", dtype=torch.float64) + 1) / (2 * n) if n else None
                if n:
                    w = w.to(torch.float32 if dt == "u8" else torch_dtype(dt)).view((1, 1, n, 1) if ny else (1, 1, 1, n))
                hip, tor = timed_alternately([lambda: feather_paste(src, dsts[0], ramp=(ny, nx)), lambda: torch_paste(src, dsts[1], (ny, nx), w)],
                                             warmup, iters)
                total = B * 3 * H * W
                under = B * 3 * (ny * W if ny else H * nx)
                nbytes = e * (3 * under + 2 * (total - under))
                diff = (dsts[0][0, :, ::8, ::8].float() - dsts[1][0, :, ::8, ::8].float()).abs().max()
                rows.append({"step": "paste", "dtype": dt, "images": [B, H, W], "ramp": [ny, nx], "warmup": warmup, "iters": iters, "bytes": nbytes,
                             "hip": stats(hip), "torch": stats(tor), "torch_over_hip": stats(tor)["median_ms"] / stats(hip)["median_ms"],
                             "hip_tbytes_per_s": nbytes / (stats(hip)["median_ms"] * 1e-3) / 1e12,
                             "max_abs_difference_sampled": float(diff) / (255.0 if dt == "u8" else 1.0)})
            del src, dsts
            torch.cuda.empty_cache()
    return rows


def headline_model():
    import torch

    from ultrazoom_amd import MewZoom

    torch.manual_seed(0)
    return MewZoom(**HEADLINE).to("cuda", torch.bfloat16).eval()


def step_whole(shape, warmup, iters):
    import torch

    from ultrazoom_amd import tiling

    B, H, W = shape
    m = headline_model()
    r = m.upscale_ratio
    need = tiling.receptive_field(m._cfg)
    with torch.inference_mode():
        x = rgb_image(B, H, W, "bf16")
        outs = [torch.empty((B, 3, r * H, r * W), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
        runs = [lambda: tiling.upscale_tiled(m, x, tile=(1024, 1024), out=outs[0]),
                lambda: tiling.upscale_feathered(m, x, tile=(1024, 1024), halo=32, out=outs[1]),
                lambda: tiling.upscale_feathered(m, x, tile=(512, 512), halo=32, out=outs[2])]
        exact, f1024, f512 = (stats(ms) for ms in timed_alternately(runs, warmup, iters))
        # the pastes of one run of each feathered plan: events around every call of tiling.feather_paste
        paste_ms = []
        plain = tiling.feather_paste
        for run in runs[1:]:
            events = []

            def timed(src, dst, ramp=(0, 0)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                plain(src, dst, ramp)
                e1.record()
                events.append((e0, e1))
                return dst

            tiling.feather_paste = timed
            try:
                run()
            finally:
                tiling.feather_paste = plain
            torch.cuda.synchronize()
            paste_ms.append((len(events), sum(e0.elapsed_time(e1) for e0, e1 in events)))
        err = [float((o.float() - outs[0].float()).abs().max()) for o in outs[1:]]
    work = {"exact_1024": tiling.tile_work(H, W, (1024, 1024), need), "feathered_1024": tiling.tile_work(H, W, (1024, 1024), 32),
            "feathered_512": tiling.tile_work(H, W, (512, 512), 32)}
    res = {"step": "whole", "model": "4X-96 (headline), synthetic weights", "dtype": "bf16", "images": [B, H, W], "warmup": warmup, "iters": iters,
           "receptive_field": need, "upscale_tiled_1024": exact, "upscale_feathered_1024_halo32": f1024, "upscale_feathered_512_halo32": f512,
           "tile_work": work}
    for name, got, (count, ms), dev in (("1024", f1024, paste_ms[0], err[0]), ("512", f512, paste_ms[1], err[1])):
        res[f"speedup_{name}"] = exact["median_ms"] / got["median_ms"]
        res[f"speedup_{name}_predicted_by_tile_work"] = work["exact_1024"] / work[f"feathered_{name}"]
        res[f"pastes_{name}"] = {"calls": count, "summed_ms": ms, "share_of_run": ms / got["median_ms"]}
        res[f"max_abs_against_exact_{name}"] = dev
    return [res]


def step_deviation(shape, warmup, iters):
    import torch

    from ultrazoom_amd import tiling

    B, H, W = shape
    m = headline_model()
    rows = []
    with torch.inference_mode():
        x = rgb_image(B, H, W, "bf16")
        full = m.upscale(x).float()

        def against(y):
            d = y.float() - full
            mse = float((d * d).mean())
            return {"max_abs": float(d.abs().max()), "psnr_db": 10.0 * math.log10(1.0 / mse) if mse > 0 else None}

        for halo in HALOS:
            blended = tiling.upscale_feathered(m, x, tile=(512, 512), halo=halo)
            hard = tiling.upscale_feathered(m, x, tile=(512, 512), halo=halo, overlap=0)
            rows.append({"step": "deviation", "model": "4X-96 (headline), synthetic weights", "dtype": "bf16", "images": [B, H, W], "tile": 512,
                         "halo": halo, "overlap": halo // 2, "blended": against(blended), "hard_cut": against(hard)})
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "feather_bench.json"))
    ap.add_argument("--step", choices=("paste", "whole", "deviation"))
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds for one step")
    a = ap.parse_args()
    if a.step:
        for row in {"paste": step_paste, "whole": step_whole, "deviation": step_deviation}[a.step](tuple(a.shape), a.warmup, a.iters):
            print(json.dumps(row), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "paste": [], "whole": None, "deviation": [], "stopped": None}

    def finish(why=None):
        result["stopped"] = why
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps({"paste": result["paste"], "whole": result["whole"], "deviation": result["deviation"]}, indent=1))
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

    rows, err = run("paste", PASTE, a.warmup, a.iters)
    if err:
        return finish(err)
    for got in rows:
        result["paste"].append({"dtype": got["dtype"], "images": got["images"], "ramp": got["ramp"], "hip_ms": got["hip"]["median_ms"],
                                "torch_ms": got["torch"]["median_ms"], "torch_over_hip": got["torch_over_hip"], "bytes": got["bytes"],
                                "hip_tbytes_per_s": got["hip_tbytes_per_s"], "hip_fraction_of_stream_rate": got["hip_tbytes_per_s"] / stream,
                                "max_abs_difference_sampled": got["max_abs_difference_sampled"]})
    rows, err = run("whole", WHOLE, 1, min(a.iters, 3))
    if err:
        return finish(err)
    result["whole"] = rows[0]
    rows, err = run("deviation", DEVIATION, 0, 1)
    if err:
        return finish(err)
    result["deviation"] = rows
    return finish()


if __name__ == "__main__":
    sys.exit(main())
