"""Writes tests/golden/d1_jpeg_codec.npz: three small seeded uint8 images (smooth gradients and waves plus noise) and what a real codec
makes of them -- Pillow's JPEG encoder and decoder (libjpeg-turbo) at their default settings (4:2:0 chroma subsampling, the standard
tables scaled by the quality, no optimisation that changes the pixels), at qualities 20, 50, 90 and 100.  The tests read the file,
never Pillow.  Run from the repository root:  python tests/golden/make_degrade_golden.py

Keys: in_<i> [3, H, W] uint8;  out_<i>_q<quality> [3, H, W] uint8."""

import io
from pathlib import Path

import numpy as np
from PIL import Image

SIZES = ((37, 45), (64, 64), (48, 80))
QUALITIES = (20, 50, 90, 100)


def image(i: int, H: int, W: int) -> np.ndarray:
    rng = np.random.default_rng(100 + i)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = []
    for c in range(3):
        fy, fx, ph = rng.uniform(0.02, 0.25, 3)
        smooth = 0.5 + 0.25 * np.sin(fy * y + 2.0 * ph * c) * np.cos(fx * x + ph) + 0.2 * (x / W - y / H) * (1 - c / 2)
        planes.append(smooth + rng.normal(0.0, 0.04, (H, W)))
    return (np.clip(np.stack(planes), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def main() -> None:
    data = {}
    for i, (H, W) in enumerate(SIZES):
        x = image(i, H, W)
        data[f"in_{i}"] = x
        for q in QUALITIES:
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(x.transpose(1, 2, 0)), "RGB").save(buf, format="JPEG", quality=q)
            buf.seek(0)
            data[f"out_{i}_q{q}"] = np.asarray(Image.open(buf).convert("RGB")).transpose(2, 0, 1).copy()
    path = Path(__file__).resolve().parent / "d1_jpeg_codec.npz"
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
