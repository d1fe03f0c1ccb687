#!/usr/bin/env python3
"""Times the dihedral / self-ensemble kernels (`mz_dihedral`, `mz_ensemble_add`) against torch's own composition on the same CUDA tensors,
and the whole `upscale_ensemble` of the headline model against 8 plain passes and against the torch-composed ensemble.

    python tools/ensemble_bench.py --out profiles/ensemble_bench.json

The driver never touches the GPU: every step is a child process of its own under its own `timeout -k 10`, and the first step that
fails, faults or runs out of time ends the run (what was measured until then is written).  Steps: the box's streaming rate
(tools/microbench/mb_stream, built here with `hipcc --offload-arch=gfx950 -O3` when it is missing; the best variant counts), then

  per orientation   bf16 and u8, [1,3,2160,3840] and [16,3,4320,7680], every k: `mz_dihedral`, `mz_ensemble_add` (adding, not the first
                    store) and torch's `acc += T(y, inverse(k))` on a float32 accumulator.  HIP events around `iters` calls after warm-up.
                    Algorithmic bytes: every element read once and written once (dihedral: 2 e an element), plus 4 bytes read and 4
                    written per accumulator element (add: e + 8).
  whole ensemble    the headline model (4X 96ch/40L, bf16), 4 x 1080x1920, n = 8: `upscale_ensemble`, 8 x `upscale` of the same batch (into one output tensor),
                    and the torch composition (`flip` / `transpose(...).contiguous()` at both ends, a float32 running sum, the finish).

Acceptance (margin 1.0, the same run, the same tensors): for every orientation the HIP add is not slower than torch's; the whole HIP
ensemble is not slower than the torch-composed one."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

SHAPES = [(1, 2160, 3840), (16, 4320, 7680)]  # the RESULT's shape
DTYPES = ("bf16", "u8")
MB_STREAM = REPO / "tools" / "microbench" / "mb_stream"
HEADLINE = dict(upscale_ratio=4, primary_channels=96, primary_layers=8, secondary_channels=192, secondary_layers=8, tertiary_channels=384,
                tertiary_layers=8, quaternary_channels=768, quaternary_layers=16, hidden_ratio=2, num_deg_features=3)
WHOLE = (4, 1080, 1920)


def T(x, k):
    if k & 2:
        x = x.flip(2)
    if k & 1:
        x = x.flip(3)
    if k & 4:
        x = x.transpose(2, 3)
    return x


def inverse(k):
    return k if k < 4 else 4 | ((k & 1) << 1) | ((k & 2) >> 1)


def image(B, H, W, dt):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    if dt == "u8":
        x = torch.empty((B, 3, H, W), device="cuda", dtype=torch.uint8)
        for b in range(B):
            x[b].random_(0, 256, generator=g)
        return x
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
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def step_orientations(dt: str, B: int, H: int, W: int, warmup: int, iters: int) -> list:
    """One row per orientation: the three timings on one set of tensors."""
    import torch

    from ultrazoom_amd import _ffi
    from ultrazoom_amd.ensemble import dihedral

    stream = torch.cuda.current_stream().cuda_stream
    base = image(B, H, W, dt)  # every y is a view of one allocation's worth of pixels, in its own orientation's shape
    e = base.element_size()
    n = base.numel()
    elem = _ffi.elem_code(base.dtype)
    need = _ffi.ensemble_workspace_bytes(B, H, W)
    acc = torch.zeros((B, 3, H, W), dtype=torch.float32, device="cuda")
    out = torch.empty(n, dtype=base.dtype, device="cuda")
    rows = []
    for k in range(8):
        y = base.view(B, 3, W, H) if k & 4 else base  # dense, in orientation k's shape
        hk, wk = y.shape[2], y.shape[3]
        ok = out.view(B, 3, wk, hk) if k & 4 else out.view(B, 3, hk, wk)
        ms_dihedral = timed(lambda: dihedral(y, k, out=ok), warmup, iters)
        ms_add = timed(lambda: _ffi.ensemble_add(y.data_ptr(), y.stride(), elem, B, H, W, k, False, acc.data_ptr(), need, stream), warmup, iters)

        def torch_add():
            acc.add_(T(y, inverse(k)))

        with torch.inference_mode():
            ms_torch = timed(torch_add, warmup, iters)
        rows.append({
            "step": "orientations", "dtype": dt, "shape": [B, 3, H, W], "k": k, "warmup": warmup, "iters": iters,
            "dihedral_ms": ms_dihedral, "add_ms": ms_add, "torch_add_ms": ms_torch,
            "dihedral_bytes": 2 * e * n, "add_bytes": (e + 8) * n,
            "dihedral_tbytes_per_s": 2 * e * n / (ms_dihedral * 1e-3) / 1e12, "add_tbytes_per_s": (e + 8) * n / (ms_add * 1e-3) / 1e12,
            "torch_over_hip_add": ms_torch / ms_add,
        })
    return rows


def step_whole(kind: str, warmup: int, iters: int) -> list:
    import torch

    from ultrazoom_amd import MewZoom

    B, H, W = WHOLE
    torch.manual_seed(0)
    m = MewZoom(**HEADLINE).to("cuda", torch.bfloat16).eval()
    x = image(B, H, W, "bf16")
    r = m.upscale_ratio
    res = {"step": kind, "dtype": "bf16", "shape": [B, 3, H, W], "n": 8, "warmup": warmup, "iters": iters}
    out = torch.empty((B, 3, r * H, r * W), dtype=x.dtype, device="cuda")
    if kind == "hip_ensemble":
        fn = lambda: m.upscale_ensemble(x, n=8, out=out)  # noqa: E731
    elif kind == "plain_passes":
        def fn():
            for _ in range(8):
                m.upscale_into(x, out)
    else:
        def fn():  # the composition a user writes in torch today
            acc = None
            for k in range(8):
                y = T(m.upscale(T(x, k).contiguous()), inverse(k)).float()
                acc = y.contiguous() if acc is None else acc.add_(y)
            out.copy_((acc * 0.125).clamp_(0, 1))
    with torch.inference_mode():
        res["ms"] = timed(fn, warmup, iters)
    res["checksum"] = float(out[0, :, ::16, ::16].float().mean())
    return [res]


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
    ap.add_argument("--out", default=str(REPO / "profiles" / "ensemble_bench.json"))
    ap.add_argument("--step", choices=["orientations", "hip_ensemble", "plain_passes", "torch_ensemble"])
    ap.add_argument("--dtype", choices=DTYPES)
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="timed calls of a per-orientation step; the whole ensemble runs a tenth of them")
    ap.add_argument("--limit", type=int, default=240, help="seconds for one step")
    a = ap.parse_args()
    if a.step == "orientations":
        print(json.dumps(step_orientations(a.dtype, *a.shape, a.warmup, a.iters)), flush=True)
        return 0
    if a.step:
        print(json.dumps(step_whole(a.step, 1, max(2, a.iters // 10))), flush=True)
        return 0

    result = {"stream": None, "stream_tbytes_per_s": None, "steps": [], "summary": [], "whole": None, "acceptance": None, "stopped": None}

    def write():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")

    def finish(why=None):
        result["stopped"] = why
        write()
        print(json.dumps({"summary": result["summary"], "whole": result["whole"], "acceptance": result["acceptance"]}, indent=1))
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
    me = [sys.executable, str(Path(__file__).resolve()), "--warmup", a.warmup, "--iters", a.iters]
    worst_add = None
    for B, H, W in SHAPES:
        for dt in DTYPES:
            rows, err = child(me + ["--step", "orientations", "--dtype", dt, "--shape", B, H, W], a.limit)
            if err:  # recorded, and the run ends: nothing more is started on a GPU that may have faulted
                result["steps"].append({"step": "orientations", "dtype": dt, "shape": [B, 3, H, W], "ran": False, "why": err})
                return finish(f"orientations {dt} {B} x {H} x {W}: {err}")
            result["steps"] += rows
            for r in rows:
                result["summary"].append({
                    "dtype": dt, "shape": [B, 3, H, W], "k": r["k"], "dihedral_ms": r["dihedral_ms"], "add_ms": r["add_ms"],
                    "torch_add_ms": r["torch_add_ms"], "torch_over_hip_add": r["torch_over_hip_add"],
                    "dihedral_fraction_of_stream_rate": r["dihedral_tbytes_per_s"] / stream,
                    "add_fraction_of_stream_rate": r["add_tbytes_per_s"] / stream,
                })
                worst_add = r["torch_over_hip_add"] if worst_add is None else min(worst_add, r["torch_over_hip_add"])
            write()  # the file grows while the run goes on
    whole = {}
    for kind in ("hip_ensemble", "plain_passes", "torch_ensemble"):
        rows, err = child(me + ["--step", kind], max(a.limit, 420))
        if err:
            result["steps"].append({"step": kind, "ran": False, "why": err})
            return finish(f"{kind}: {err}")
        result["steps"] += rows
        whole[kind + "_ms"] = rows[0]["ms"]
        write()
    whole["overhead_over_8_passes"] = whole["hip_ensemble_ms"] / whole["plain_passes_ms"] - 1.0
    whole["torch_over_hip"] = whole["torch_ensemble_ms"] / whole["hip_ensemble_ms"]
    result["whole"] = whole
    result["acceptance"] = {"worst_torch_over_hip_add": worst_add, "every_add_not_slower_than_torch": worst_add >= 1.0,
                            "whole_torch_over_hip": whole["torch_over_hip"], "whole_not_slower_than_torch": whole["torch_over_hip"] >= 1.0}
    return finish()


if __name__ == "__main__":
    sys.exit(main())
