#!/usr/bin/env python3
"""Times the YCbCr kernels of any depth and subsampling, in the manner of tools/yuv_bench.py: (a) `ultrazoom_amd.ycbcr_to_rgb` and
`rgb_to_ycbcr` (`mz_ycbcr_to_rgb`, `mz_rgb_to_ycbcr`) on 16 frames of 2160 x 3840 inside frame buffers of four formats -- P010 (10 bits,
high, semi-planar 4:2:0), yuv420p10le (low, planar), 10-bit planar 4:2:2 and 8-bit planar 4:4:4 -- RGB as bf16 and f32, against the torch
composition a user would write for the same conversion on the same tensors (the int16 view of the uint16 words widened and shifted,
`F.interpolate(..., mode="bilinear")` for the chroma of "center" siting, the matrix as tensor expressions, `avg_pool2d` for the way
back), against the box's streaming rate, and against the 8-bit 4:2:0 entries (`yuv420_to_rgb`, `rgb_to_yuv420` on NV12) timed in the
same run; (b) `MewZoom.upscale_ycbcr` on 16 P010 frames of 1080 x 1920 against `upscale` on the equivalent RGB batch, headline model, bf16.

    python tools/ycbcr_bench.py --out profiles/ycbcr_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  HIP events around every single call after
warm-up; the MEDIAN of the calls counts, the kernel and the composition timed alternately.  Algorithmic bytes of (a) per pixel:
(1 + 2 / (sub_w * sub_h)) * sample bytes + 3 * (bytes of an RGB element).

CONDITIONS: no case of (a) is slower than its composition (`torch_over_hip` >= 1.0); (b)'s added time stays within three times the
conversions' bytes at the measured streaming rate (the budget rule of tools/yuv_bench.py).  `condition_holds` records both and the exit
status follows it.  The fractions of the streaming rate are recorded, not fixed in advance."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from yuv_bench import HEADLINE, MB_STREAM, child, rgb_image, stats, timed_alternately, torch_dtype  # noqa: E402

FRAMES = (16, 2160, 3840)
WHOLE = (16, 1080, 1920)
DTYPES = ("bf16", "f32")
DIRECTIONS = ("to_rgb", "to_ycbcr")
# name: depth, align, subsampling, layout, (sub_h, sub_w)
FORMATS = {
    "p010": (10, "high", "420", "semiplanar", (2, 2)),
    "yuv420p10le": (10, "low", "420", "planar", (2, 2)),
    "yuv422p10le": (10, "low", "422", "planar", (1, 2)),
    "yuv444p": (8, "low", "444", "planar", (1, 1)),
    "nv12 (the 8-bit 4:2:0 entries)": (8, "low", "420", "semiplanar", (2, 2)),
}
BASELINE = "nv12 (the 8-bit 4:2:0 entries)"
PARAMS = dict(matrix="bt709", range="limited", siting="center")  # "center": the siting F.interpolate and avg_pool2d compute
KR, KB = 0.2126, 0.0722


def frame_elems(H, W, sub):
    sh, sw = sub
    return H * W + 2 * (H // sh) * (W // sw)


def frames(B, H, W, depth, sub, seed=1):
    """a [B, n] uint8 / uint16 buffer of random words (every bit: the formats read what they read)"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    n = frame_elems(H, W, sub)
    if depth == 8:
        buf = torch.empty((B, n), device="cuda", dtype=torch.uint8)
        for b in range(B):
            buf[b].random_(0, 256, generator=g)
        return buf
    raw = torch.empty((B, n), device="cuda", dtype=torch.int16)
    for b in range(B):
        raw[b] = torch.randint(0, 65536, (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)  # (keeps the low 16 bits)
    return raw.view(torch.uint16)


def codes_of(t, depth, align):
    """float32 code values of a plane of stored words, by the operations torch has for them"""
    import torch

    if t.dtype == torch.uint8:
        return t.float()
    v = t.view(torch.int16).int() & 0xFFFF
    v = (v >> (16 - depth)) if align == "high" else (v & (2 ** depth - 1))
    return v.float()


def store_codes(plane, v, depth, align):
    """float32 code values (clamped, + 0.5) into a plane of stored words"""
    import torch

    if plane.dtype == torch.uint8:
        plane.copy_(v)
        return
    w = v.int()
    if align == "high":
        w = w << (16 - depth)
    plane.view(torch.int16).copy_(w)  # (int32 -> int16 keeps the low 16 bits)


def torch_to_rgb(y, cb, cr, out, depth, align, sub):
    """the composition a user writes today: the words widened and shifted, bilinear chroma, the matrix as tensor expressions"""
    import torch
    import torch.nn.functional as F

    s = float(2 ** (depth - 8))
    kg = 1.0 - KR - KB
    yn = (codes_of(y, depth, align) - 16.0 * s) / (219.0 * s)
    chroma = []
    for c in (cb, cr):
        c = codes_of(c, depth, align)
        if sub != (1, 1):
            c = F.interpolate(c, scale_factor=(float(sub[0]), float(sub[1])), mode="bilinear", align_corners=False)
        chroma.append((c - 128.0 * s) / (224.0 * s))
    cbn, crn = chroma
    rgb = torch.cat([yn + 2 * (1 - KR) * crn, yn - (2 * KR * (1 - KR) / kg) * crn - (2 * KB * (1 - KB) / kg) * cbn, yn + 2 * (1 - KB) * cbn], dim=1)
    out.copy_(rgb.clamp_(0, 1))


def torch_to_ycbcr(x, y, cb, cr, depth, align, sub):
    import torch.nn.functional as F

    s, top = float(2 ** (depth - 8)), float(2 ** depth - 1)
    v = x.float()
    r, g, b = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    lum = KR * r + (1.0 - KR - KB) * g + KB * b
    store_codes(y, (lum * (219.0 * s) + 16.0 * s).clamp_(0, top).add_(0.5), depth, align)
    for plane, p in ((cb, (b - lum) * (0.5 / (1 - KB))), (cr, (r - lum) * (0.5 / (1 - KR)))):
        if sub != (1, 1):
            p = F.avg_pool2d(p, sub)
        store_codes(plane, (p * (224.0 * s) + 128.0 * s).clamp_(0, top).add_(0.5), depth, align)


def step_convert(direction: str, name: str, dt: str, B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch

    from ultrazoom_amd import frame_planes, nv12_planes, rgb_to_ycbcr, rgb_to_yuv420, ycbcr_to_rgb, yuv420_to_rgb

    depth, align, subsampling, layout, sub = FORMATS[name]
    elem = torch.empty((), dtype=torch_dtype(dt)).element_size()
    sample = 2 if depth > 8 else 1
    nbytes = B * frame_elems(H, W, sub) * sample + B * 3 * H * W * elem
    res = {"step": direction, "format": name, "dtype": dt, "frames": [B, H, W], "warmup": warmup, "iters": iters, "bytes": nbytes,
           "bytes_per_pixel": (1 + 2 / (sub[0] * sub[1])) * sample + 3 * elem, **PARAMS}
    kw = dict(depth=depth, align=align, subsampling=subsampling, **PARAMS)
    old = name == BASELINE  # the parent's unchanged entries on NV12 views

    def cut(buf):
        return nv12_planes(buf.view(B, H * 3 // 2, W)) if old else frame_planes(buf, H, W, layout=layout, subsampling=subsampling)

    with torch.inference_mode():
        if direction == "to_rgb":
            planes = cut(frames(B, H, W, depth, sub))
            out_hip, out_torch = (torch.empty((B, 3, H, W), dtype=torch_dtype(dt), device="cuda") for _ in range(2))
            hip_fn = (lambda: yuv420_to_rgb(*planes, out=out_hip, **PARAMS)) if old else (lambda: ycbcr_to_rgb(*planes, out=out_hip, **kw))
            hip, tor = timed_alternately([hip_fn, lambda: torch_to_rgb(*planes, out_torch, depth, align, sub)], warmup, iters)
            res["max_abs_difference_sampled"] = float((out_hip[0, :, ::8, ::8].float() - out_torch[0, :, ::8, ::8].float()).abs().max())
        else:
            x = rgb_image(B, H, W, dt)
            buf_hip, buf_torch = (frames(B, H, W, depth, sub, seed=3) for _ in range(2))
            p_hip, p_torch = cut(buf_hip), cut(buf_torch)
            hip_fn = (lambda: rgb_to_yuv420(x, out=p_hip, **PARAMS)) if old else (lambda: rgb_to_ycbcr(x, out=p_hip, **kw))
            hip, tor = timed_alternately([hip_fn, lambda: torch_to_ycbcr(x, *p_torch, depth, align, sub)], warmup, iters)
            a, b = (codes_of(t[0, ::4 * 1024 + 4], depth, align) for t in (buf_hip, buf_torch))
            res["max_code_difference_sampled"] = float((a - b).abs().max())
    res["hip"], res["torch"] = stats(hip), stats(tor)
    res["hip_tbytes_per_s"] = nbytes / (res["hip"]["median_ms"] * 1e-3) / 1e12
    res["hip_tbytes_per_s_range"] = [nbytes / (res["hip"][k] * 1e-3) / 1e12 for k in ("max_ms", "min_ms")]
    res["torch_over_hip"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
    return res


def step_whole(B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch

    from ultrazoom_amd import MewZoom, frame_planes, ycbcr_to_rgb

    torch.manual_seed(0)
    m = MewZoom(**HEADLINE).to("cuda", torch.bfloat16).eval()
    r = m.upscale_ratio
    depth, align, subsampling, layout, sub = FORMATS["p010"]
    with torch.inference_mode():
        src = frame_planes(frames(B, H, W, depth, sub), H, W, layout=layout, subsampling=subsampling)
        dst_buf = frames(B, r * H, r * W, depth, sub, seed=3)
        dst = frame_planes(dst_buf, r * H, r * W, layout=layout, subsampling=subsampling)
        kw = dict(depth=depth, align=align, subsampling=subsampling, matrix="bt709", range="limited", siting="left")
        rgb = ycbcr_to_rgb(*src, dtype=torch.bfloat16, **kw)  # the equivalent RGB batch
        out = torch.empty((B, 3, r * H, r * W), dtype=torch.bfloat16, device="cuda")
        ycc, plain = timed_alternately([lambda: m.upscale_ycbcr(*src, out=dst, **kw), lambda: m.upscale_into(rgb, out)], warmup, iters)
        checksum = float(codes_of(dst_buf[0, : 64 * 1024 : 16], depth, align).mean())
    res = {"step": "whole", "model": "4X-96 (headline)", "dtype": "bf16", "format": "p010", "frames": [B, H, W], "warmup": warmup, "iters": iters,
           "upscale_ycbcr": stats(ycc), "upscale": stats(plain)}
    res["added_ms"] = res["upscale_ycbcr"]["median_ms"] - res["upscale"]["median_ms"]
    res["conversion_bytes"] = int((3.0 + 6.0) * B * H * W + (3.0 + 6.0) * B * r * H * r * W)  # 1.5 samples of 2 bytes and 3 bf16 a pixel, each way
    res["checksum"] = checksum
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "ycbcr_bench.json"))
    ap.add_argument("--step", choices=DIRECTIONS + ("whole",))
    ap.add_argument("--format", choices=tuple(FORMATS))
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
        print(json.dumps(step_convert(a.step, a.format, a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "convert": [], "whole": None, "condition_holds": None, "stopped": None}

    def write():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")

    def finish(why=None):
        result["stopped"] = why
        if not why:
            result["condition_holds"] = all(c["torch_over_hip"] >= 1.0 for c in result["convert"]) and result["whole"]["within_budget"]
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
        for dt in DTYPES:
            for name in FORMATS:  # the 8-bit 4:2:0 entries last: the baseline of this direction and RGB type
                got, err = run(["--step", direction, "--format", name, "--dtype", dt], FRAMES, a.warmup, a.iters)
                if err:
                    return finish(err)
                result["convert"].append({"direction": direction, "format": name, "dtype": dt, "frames": got["frames"],
                                          "bytes_per_pixel": got["bytes_per_pixel"], "hip_ms": got["hip"]["median_ms"],
                                          "torch_ms": got["torch"]["median_ms"], "torch_over_hip": got["torch_over_hip"],
                                          "hip_tbytes_per_s": got["hip_tbytes_per_s"],
                                          "hip_fraction_of_stream_rate": got["hip_tbytes_per_s"] / stream,
                                          "hip_fraction_range": [v / stream for v in got["hip_tbytes_per_s_range"]]})
            base = result["convert"][-1]["hip_fraction_of_stream_rate"]
            for c in result["convert"][-len(FORMATS):]:
                c["fraction_over_8bit_420_entry"] = c["hip_fraction_of_stream_rate"] / base
    got, err = run(["--step", "whole"], WHOLE, 1, min(a.iters, 4))
    if err:
        return finish(err)
    budget_ms = 3.0 * got["conversion_bytes"] / (stream * 1e12) * 1e3
    result["whole"] = {"model": got["model"], "dtype": "bf16", "format": "p010", "frames": got["frames"],
                       "upscale_ms": got["upscale"]["median_ms"], "upscale_ycbcr_ms": got["upscale_ycbcr"]["median_ms"],
                       "added_ms": got["added_ms"], "conversion_bytes": got["conversion_bytes"], "budget_ms": budget_ms,
                       "within_budget": got["added_ms"] <= budget_ms}
    return finish()


if __name__ == "__main__":
    sys.exit(main())
