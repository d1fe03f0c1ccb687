"""PSNR / SSIM / VIF of image batches on the MI355X: `mz_metrics` (include/mewzoom_hip.h) behind a tensor interface.

The arithmetic is that of `ultrazoom_amd/evaluate.py` (its float64 functions are the checker of these kernels), in HIP and in
float64, on the tensors as they lie in memory: any strides (channels-last, an HWC frame permuted to NCHW, BGR through a flipped
channel axis, a crop, every second image), float32 / bfloat16 / float16 / uint8 (a uint8 value v means v / 255).  Nothing is copied
and nothing here synchronises with the host: the results are float64 tensors on the device.

`luma="bt601"` or `"full"` measures the Y plane instead (`mz_metrics_luma`: the unrounded float64 Y of `ultrazoom_amd/color.py`, one
plane of metric work instead of three), `shave=k` leaves k border pixels out on every side (a narrowed view, no copy).  The protocol of
the super-resolution papers is `luma="bt601", shave=<the upscale ratio>`."""

from __future__ import annotations

import math
from typing import Iterable, Optional

import torch
from torch import Tensor

from . import _ffi

_BITS = {"psnr": _ffi.MZ_METRIC_PSNR, "ssim": _ffi.MZ_METRIC_SSIM, "vif": _ffi.MZ_METRIC_VIF}


def shaved(x: Tensor, shave: int) -> Tensor:
    """`x[..., k:H-k, k:W-k]`, a view: the border crop of the super-resolution protocol."""
    if isinstance(shave, bool) or not isinstance(shave, int) or shave < 0:
        raise ValueError(f"shave is a number of border pixels >= 0, got {shave!r}")
    if x.dim() < 2:
        raise ValueError(f"expected a [B, 3, H, W] tensor, got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if 2 * shave >= min(H, W):
        raise ValueError(f"shave={shave} leaves nothing of {H} x {W} pixels")
    return x[..., shave:H - shave, shave:W - shave] if shave else x


def _check_sizes(which, H: int, W: int) -> None:
    for name, least in _ffi.MZ_METRIC_MIN_SIZE.items():
        if name in which and min(H, W) < least:
            raise ValueError(f"{name.upper()} needs images of at least {least} x {least} pixels, got {(H, W)}")


def image_metrics(pred: Tensor, target: Tensor, *, which: Iterable[str] = ("psnr", "ssim", "vif"), data_range: Optional[float] = None,
                  sigma_n_sq: float = 2.0, luma: Optional[str] = None, shave: int = 0) -> dict:
    """Per-image sums of the requested metrics of two logical [B, 3, H, W] CUDA tensors of one dtype, as float64 device tensors [B]:
    "psnr" -> "sq_err" (sum of squared differences) and "numel"; "ssim" -> "ssim" (`evaluate.ssim_per_image`; `data_range=None` = the
    larger range of the two batches); "vif" -> "vif" (`evaluate.vif_per_image`).
    Floating-point values are taken as they are and not range-checked: [0, 1] images and 0..255 images are both measured on their own
    scale (uint8 always means v / 255); NaN or infinite pixels propagate into the sums.
    `luma`: None measures the three RGB planes; "bt601" or "full" the float64 Y plane of that standard ("numel" is then H W, "vif" the
    value of the one plane, `data_range=None` the range of the Y planes).  `shave=k` measures `[..., k:H-k, k:W-k]` of both tensors; the
    sizes SSIM and VIF need are those left after the shave."""
    which = tuple(which)
    standard = None if luma is None else _ffi.luma_standard(luma)
    unknown = [w for w in which if w not in _BITS]
    if unknown or not which:
        raise ValueError(f"which holds names out of 'psnr', 'ssim', 'vif', got {which}")
    if shave:  # what the shave leaves is an error of the arguments: found on the shapes alone, before the tensors are looked at
        _check_sizes(which, *shaved(pred, shave).shape[-2:])
    elem, B, _, _ = _ffi.check_image_batch(pred, "metrics", target, names=("pred", "target"))
    pred, target = shaved(pred, shave), shaved(target, shave)
    H, W = pred.shape[-2:]
    _check_sizes(which, H, W)
    bits = sum(_BITS[w] for w in set(which))
    need = _ffi.metrics_workspace_bytes if luma is None else _ffi.metrics_luma_workspace_bytes
    with _ffi.image_frame(pred, need=lambda: need(B, H, W, bits)) as (_, ws, stream):
        out = torch.zeros((B, _ffi.MZ_METRIC_SLOTS), dtype=torch.float64, device=pred.device)
        rng = -1.0 if data_range is None else float(data_range)
        views = (*_ffi.pair(pred), *_ffi.pair(target))
        if luma is None:
            _ffi.metrics(*views, elem, B, H, W, bits, rng, float(sigma_n_sq), out.data_ptr(), *ws, stream)
        else:
            _ffi.metrics_luma(*views, elem, B, H, W, bits, standard, rng, float(sigma_n_sq), out.data_ptr(), *ws, stream)
    res = {}
    if "psnr" in which:
        res["sq_err"], res["numel"] = out[:, 0], out[:, 1]
    if "ssim" in which:
        res["ssim"] = out[:, 6] / out[:, 7]
    if "vif" in which:
        # 0 / 0 = NaN where the torch restatement has it; with luma: the one plane, slot 8 / slot 11
        res["vif"] = (out[:, 8:11] / out[:, 11:14]).mean(dim=1) if luma is None else out[:, 8] / out[:, 11]
    return res


class MetricsAccumulator:
    """The three accumulators of `evaluate.py` (PSNR: one global MSE over all updates; SSIM, VIF: mean of the per-image values) over
    `image_metrics`.  The running sums stay on the device; `compute()` reads them, once.  VIF skips updates with images below 41 pixels,
    as `evaluate()` does (with `shave`: below 41 after the shave).  `luma` and `shave` as for `image_metrics`."""

    def __init__(self, psnr_range: float = 1.0, data_range: Optional[float] = None, sigma_n_sq: float = 2.0, luma: Optional[str] = None,
                 shave: int = 0):
        self.psnr_range, self.data_range, self.sigma_n_sq = float(psnr_range), data_range, float(sigma_n_sq)
        if luma is not None:
            _ffi.luma_standard(luma)
        self.luma, self.shave = luma, shave
        self.reset()

    def reset(self) -> None:
        self._sums = None  # device float64 [4]: squared error, elements, SSIM total, VIF total
        self.ssim_n = 0
        self.vif_n = 0

    def update(self, pred: Tensor, target: Tensor) -> None:
        with_vif = min(shaved(pred, self.shave).shape[-2:]) >= _ffi.MZ_METRIC_MIN_SIZE["vif"]
        r = image_metrics(pred, target, which=("psnr", "ssim", "vif") if with_vif else ("psnr", "ssim"), data_range=self.data_range,
                          sigma_n_sq=self.sigma_n_sq, luma=self.luma, shave=self.shave)
        vif = r["vif"].sum() if with_vif else torch.zeros((), dtype=torch.float64, device=pred.device)
        add = torch.stack([r["sq_err"].sum(), r["numel"].sum(), r["ssim"].sum(), vif])
        self._sums = add if self._sums is None else self._sums + add
        self.ssim_n += pred.shape[0]
        self.vif_n += pred.shape[0] if with_vif else 0

    def compute(self, extra: Optional[Tensor] = None):
        """The metrics; with `extra` (a float64 device vector the caller accumulated next to them) `(metrics, extra values)`, both
        from the same single read."""
        if self._sums is None:
            res = {"psnr": float("nan"), "ssim": float("nan"), "vif": None}
            return res if extra is None else (res, extra.tolist())
        values = (self._sums if extra is None else torch.cat([self._sums, extra.to(self._sums.device, torch.float64)])).tolist()  # the one read
        sq, n, ssim, vif = values[:4]
        mse = sq / n
        psnr = float("inf") if mse == 0.0 else 10.0 * math.log10(self.psnr_range**2 / mse)
        res = {"psnr": psnr, "ssim": ssim / self.ssim_n, "vif": vif / self.vif_n if self.vif_n else None}
        return res if extra is None else (res, values[4:])
