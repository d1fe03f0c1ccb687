"""PSNR / SSIM / VIF of image batches on the MI355X: `mz_metrics` (include/mewzoom_hip.h) behind a tensor interface.

The arithmetic is that of `ultrazoom_amd/evaluate.py` (its float64 functions are the checker of these kernels), in HIP and in
float64, on the tensors as they lie in memory: any strides (channels-last, an HWC frame permuted to NCHW, BGR through a flipped
channel axis, a crop, every second image), float32 / bfloat16 / float16 / uint8 (a uint8 value v means v / 255).  Nothing is copied
and nothing here synchronises with the host: the results are float64 tensors on the device."""

from __future__ import annotations

import math
from typing import Iterable, Optional

import torch
from torch import Tensor

from . import _ffi

_BITS = {"psnr": _ffi.MZ_METRIC_PSNR, "ssim": _ffi.MZ_METRIC_SSIM, "vif": _ffi.MZ_METRIC_VIF}


def image_metrics(pred: Tensor, target: Tensor, *, which: Iterable[str] = ("psnr", "ssim", "vif"), data_range: Optional[float] = None,
                  sigma_n_sq: float = 2.0) -> dict:
    """Per-image sums of the requested metrics of two logical [B, 3, H, W] CUDA tensors of one dtype, as float64 device tensors [B]:
    "psnr" -> "sq_err" (sum of squared differences) and "numel"; "ssim" -> "ssim" (`evaluate.ssim_per_image`; `data_range=None` = the
    larger range of the two batches); "vif" -> "vif" (`evaluate.vif_per_image`).
    Floating-point values are taken as they are and not range-checked: [0, 1] images and 0..255 images are both measured on their own
    scale (uint8 always means v / 255); NaN or infinite pixels propagate into the sums."""
    which = tuple(which)
    unknown = [w for w in which if w not in _BITS]
    if unknown or not which:
        raise ValueError(f"which holds names out of 'psnr', 'ssim', 'vif', got {which}")
    elem, B, H, W = _ffi.check_image_batch(pred, "metrics", target, names=("pred", "target"))
    if "ssim" in which and min(H, W) < 11:
        raise ValueError(f"SSIM needs images of at least 11 x 11 pixels, got {(H, W)}")
    if "vif" in which and min(H, W) < 41:
        raise ValueError(f"VIF needs images of at least 41 x 41 pixels, got {(H, W)}")
    bits = sum(_BITS[w] for w in set(which))
    with torch.cuda.device(pred.device):
        stream = torch.cuda.current_stream(pred.device)
        need = _ffi.metrics_workspace_bytes(B, H, W, bits)
        ws = torch.empty(need, dtype=torch.uint8, device=pred.device)
        out = torch.zeros((B, _ffi.MZ_METRIC_SLOTS), dtype=torch.float64, device=pred.device)
        _ffi.metrics(pred.data_ptr(), pred.stride(), target.data_ptr(), target.stride(), elem, B, H, W, bits,
                     -1.0 if data_range is None else float(data_range), float(sigma_n_sq), out.data_ptr(), ws.data_ptr(), need,
                     stream.cuda_stream)
    res = {}
    if "psnr" in which:
        res["sq_err"], res["numel"] = out[:, 0], out[:, 1]
    if "ssim" in which:
        res["ssim"] = out[:, 6] / out[:, 7]
    if "vif" in which:
        res["vif"] = (out[:, 8:11] / out[:, 11:14]).mean(dim=1)  # 0 / 0 = NaN where the torch restatement has it
    return res


class MetricsAccumulator:
    """The three accumulators of `evaluate.py` (PSNR: one global MSE over all updates; SSIM, VIF: mean of the per-image values) over
    `image_metrics`.  The running sums stay on the device; `compute()` reads them, once.  VIF skips updates with images below 41 pixels,
    as `evaluate()` does."""

    def __init__(self, psnr_range: float = 1.0, data_range: Optional[float] = None, sigma_n_sq: float = 2.0):
        self.psnr_range, self.data_range, self.sigma_n_sq = float(psnr_range), data_range, float(sigma_n_sq)
        self.reset()

    def reset(self) -> None:
        self._sums = None  # device float64 [4]: squared error, elements, SSIM total, VIF total
        self.ssim_n = 0
        self.vif_n = 0

    def update(self, pred: Tensor, target: Tensor) -> None:
        with_vif = min(pred.shape[-2:]) >= 41
        r = image_metrics(pred, target, which=("psnr", "ssim", "vif") if with_vif else ("psnr", "ssim"), data_range=self.data_range,
                          sigma_n_sq=self.sigma_n_sq)
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
