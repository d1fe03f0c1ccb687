#!/usr/bin/env python3
"""Times the degradation kernels (`ultrazoom_amd.degrade`: gaussian_blur at sigma 1.0, gaussian_noise, jpeg at quality 50) on CUDA
tensors, bf16 and uint8, and for the blur torch's own depthwise `conv2d` (reflect `F.pad`, then the 7 x 7 kernel, as torchvision's
`gaussian_blur` does it) on the same tensors.

    python tools/degrade_bench.py --out profiles/degrade_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  Steps: the box's streaming rate
(tools/microbench/mb_stream, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing; the best variant counts), then per
operation and element type the HIP kernel, and for the blur the torch path.  Times are HIP events around `iters` calls after warm-up
calls.  Algorithmic bytes = every input element read once plus every output element written once (the JPEG workspace, 1.5 bytes a pixel
written and read again, is not counted).  Where torch has no convolution for an element type the step says so and float32 is timed."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from resize_bench import MB_STREAM, child, image, timed  # noqa: E402

# (operation, B, H, W)
CASES = [("blur", 16, 4320, 7680), ("noise", 16, 4320, 7680), ("jpeg", 16, 1080, 1920)]
DTYPES = ("bf16", "u8")
BLUR_SIGMA, NOISE_SIGMA, QUALITY = 1.0, 0.05, 50


def step(kind: str, op: str, dt: str, B: int, H: int, W: int, warmup: int, iters: int) -> dict:
    import torch
    import torch.nn.functional as F

    from ultrazoom_amd import degrade

    x = image(B, H, W, dt)
    res = {"step": kind, "op": op, "dtype": dt, "shape": [B, 3, H, W], "warmup": warmup, "iters": iters}
    if kind == "hip":
        out = torch.empty_like(x)
        fn = {"blur": lambda: degrade.gaussian_blur(x, BLUR_SIGMA, out=out), "noise": lambda: degrade.gaussian_noise(x, NOISE_SIGMA, seed=1, out=out),
              "jpeg": lambda: degrade.jpeg(x, QUALITY, out=out)}[op]
        ms, out = timed(fn, warmup, iters)
        res["checksum"] = float(out[0].float().mean()) / (255.0 if dt == "u8" else 1.0)
    else:
        assert op == "blur"
        half = int(3 * BLUR_SIGMA)

        def torch_path(v):
            j = torch.arange(-half, half + 1, device="cuda", dtype=torch.float32)
            w = torch.exp(-0.5 * (j / BLUR_SIGMA) ** 2)
            w = (w / w.sum()).to(v.dtype)
            k = (w[:, None] * w[None, :]).expand(3, 1, 2 * half + 1, 2 * half + 1).contiguous()
            return F.conv2d(F.pad(v, (half, half, half, half), mode="reflect"), k, groups=3)

        with torch.inference_mode():
            try:
                torch_path(x[:1, :, :64, :64])
                torch.cuda.synchronize()
                src = x
            except RuntimeError as e:  # no convolution of this element type in torch's HIP build: float32 stands in, and the row says so
                res["torch_dtype"] = "float32"
                res["why_float32"] = str(e).splitlines()[0][:200]
                src = torch.empty((B, 3, H, W), device="cuda", dtype=torch.float32)
                for b in range(B):
                    src[b] = x[b].float() / (255.0 if dt == "u8" else 1.0)
            ms, out = timed(lambda: torch_path(src), warmup, iters)
        res["checksum"] = float(out[0].float().mean())
    nbytes = 2 * x.numel() * x.element_size()
    res.update(ms=ms, algorithmic_bytes=nbytes, algorithmic_gbytes_per_s=nbytes / (ms * 1e-3) / 1e9)
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "degrade_bench.json"))
    ap.add_argument("--step", choices=["hip", "torch"])
    ap.add_argument("--op", choices=["blur", "noise", "jpeg"])
    ap.add_argument("--dtype", choices=DTYPES)
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.op, a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0

    result = {"stream": None, "stream_gbytes_per_s": None, "steps": [], "summary": [], "stopped": None}

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
    result["stream_gbytes_per_s"] = stream = 1e3 * max(r["TB_per_s"] for r in rows)
    for op, B, H, W in CASES:
        for dt in DTYPES:
            me = [sys.executable, str(Path(__file__).resolve()), "--op", op, "--dtype", dt, "--shape", B, H, W, "--warmup", a.warmup, "--iters", a.iters]
            pair = {}
            for kind in ("hip", "torch") if op == "blur" else ("hip",):
                rows, err = child(me + ["--step", kind], a.limit)
                if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
                    result["steps"].append({"step": kind, "op": op, "dtype": dt, "shape": [B, 3, H, W], "ran": False, "why": err})
                    return finish(f"{kind} {op} {dt} {B} x {H} x {W}: {err}")
                result["steps"] += rows
                pair[kind] = rows[0]
                write()  # the file grows while the run goes on
            row = {"op": op, "dtype": dt, "shape": [B, 3, H, W], "hip_ms": pair["hip"]["ms"],
                   "algorithmic_gbytes_per_s": pair["hip"]["algorithmic_gbytes_per_s"],
                   "fraction_of_stream_rate": pair["hip"]["algorithmic_gbytes_per_s"] / stream}
            if "torch" in pair:
                row.update(torch_ms=pair["torch"]["ms"], torch_dtype=pair["torch"].get("torch_dtype", dt),
                           torch_over_hip=pair["torch"]["ms"] / pair["hip"]["ms"])
            result["summary"].append(row)
    return finish()


if __name__ == "__main__":
    sys.exit(main())
