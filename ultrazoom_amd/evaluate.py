"""PSNR / SSIM evaluation of `MewZoom.upscale` -- the validation loop of the reference's training scripts
(pretrain.py:209-211, 301-329; fine-tune.py:231-233) without its data loaders.

The reference takes both metrics from `torchmetrics` (absent from this image), with these settings, restated here:
  * `PeakSignalNoiseRatio(data_range=1.0)`: 10 log10(1 / MSE), the squared error and the element count accumulated
    over ALL updates before the division (one global MSE, not a mean of per-image PSNRs);
  * `StructuralSimilarityIndexMeasure()` defaults: 11x11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03, the images
    reflect-padded by 5 before filtering and the border cropped again, per-image mean of the SSIM map, mean over
    images; `data_range=None` = max(range of preds, range of target) of the batch at hand.
  * `VisualInformationFidelity()` defaults (pretrain.py:211, 311-316): pixel-domain VIF (Sheikh & Bovik 2006) with
    `sigma_n_sq = 2.0`, four scales with Gaussian windows of 17, 9, 5, 3 taps (sigma = taps / 5), "valid" filtering, the
    coarser scales low-pass filtered and decimated by two; per channel, mean over channels, mean over images.  Images
    must be at least 41 pixels in both directions.
The arithmetic here is plain torch and runs wherever the tensors live; it is the evaluation harness, not part of the
kernel path, and the float64 checker of the HIP kernels that compute the same metrics (`ultrazoom_amd/metrics.py`,
`evaluate(..., backend="hip")`).  torchmetrics is absent from this image: the three metrics are checked against independent numpy / scipy
computations of the same published definitions ("parity unpinned" for the metrics themselves).

LUMA AND SHAVE.  Super-resolution papers and leaderboards (Set5, Set14, DIV2K ..) report PSNR and SSIM on the Y channel of BT.601
YCbCr with `scale` border pixels shaved off; the reference's validate.py measures RGB over the full frame, and so does everything above
by default.  `evaluate(..., luma="bt601", shave=model.upscale_ratio)` is the usual protocol: `luma` = "bt601" (studio range: MATLAB's
rgb2ycbcr, basicsr's bgr2ycbcr(y_only=True)) or "full" (JFIF / Pillow's "L") measures the float64 Y plane (`luma_plane` here,
`mz_metrics_luma` on the device; the PSNR peak stays 1.0), `shave=k` measures `[..., k:H-k, k:W-k]` of both images.  MATLAB rounds Y to
uint8 before it measures; on uint8 images that variant is
`image_metrics(rgb_to_y(p).expand(-1, 3, -1, -1), rgb_to_y(t).expand(-1, 3, -1, -1))` (`ultrazoom_amd.color.rgb_to_y`; a read view may
have stride 0)."""

from __future__ import annotations

import math
from typing import Iterable, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ._ffi import MZ_LUMA_STANDARDS, MZ_METRIC_MIN_SIZE, luma_standard, resize_filter  # names and sizes only: nothing here calls the library

VIF_MIN_SIZE = MZ_METRIC_MIN_SIZE["vif"]


class PSNR:
    def __init__(self, data_range: float = 1.0):
        self.data_range = float(data_range)
        self.reset()

    def reset(self) -> None:
        self.sq = 0.0
        self.n = 0

    def update(self, pred: Tensor, target: Tensor) -> None:
        d = pred.double() - target.double()
        self.sq += float((d * d).sum())
        self.n += d.numel()

    def compute(self) -> float:
        if self.n == 0:
            return float("nan")
        mse = self.sq / self.n
        return float("inf") if mse == 0.0 else 10.0 * math.log10(self.data_range**2 / mse)


def _gaussian_window(size: int, sigma: float, device, dtype) -> Tensor:
    x = torch.arange(size, device=device, dtype=dtype) - (size - 1) / 2.0
    g = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def ssim_per_image(pred: Tensor, target: Tensor, data_range: Optional[float] = None, size: int = 11, sigma: float = 1.5,
                   k1: float = 0.01, k2: float = 0.03) -> Tensor:
    """SSIM of each image of a [B, C, H, W] batch (Wang et al. 2004, Gaussian window)."""
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError("expected two [B, C, H, W] tensors of one shape")
    p, t = pred.double(), target.double()
    if data_range is None:
        data_range = float(max(p.max() - p.min(), t.max() - t.min()))
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    pad = (size - 1) // 2
    C = p.shape[1]
    g = _gaussian_window(size, sigma, p.device, p.dtype)
    win = (g[:, None] * g[None, :]).expand(C, 1, size, size).contiguous()

    def blur(z: Tensor) -> Tensor:
        z = F.pad(z, (pad, pad, pad, pad), mode="reflect")
        return F.conv2d(z, win, groups=C)

    mu_p, mu_t = blur(p), blur(t)
    s_pp = blur(p * p) - mu_p * mu_p
    s_tt = blur(t * t) - mu_t * mu_t
    s_pt = blur(p * t) - mu_p * mu_t
    m = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))
    m = m[..., pad:-pad, pad:-pad]  # the padded border is cropped again
    return m.reshape(m.shape[0], -1).mean(dim=1)


class SSIM:
    def __init__(self, data_range: Optional[float] = None):
        self.data_range = data_range
        self.reset()

    def reset(self) -> None:
        self.total = 0.0
        self.n = 0

    def update(self, pred: Tensor, target: Tensor) -> None:
        v = ssim_per_image(pred, target, self.data_range)
        self.total += float(v.sum())
        self.n += v.numel()

    def compute(self) -> float:
        return self.total / self.n if self.n else float("nan")


def _gaussian_kernel2d(size: int, sigma: float, device, dtype) -> Tensor:
    x = torch.arange(size, device=device, dtype=dtype) - (size - 1) / 2.0
    g = torch.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def vif_per_image(pred: Tensor, target: Tensor, sigma_n_sq: float = 2.0) -> Tensor:
    """Pixel-domain visual information fidelity of each image of a [B, C, H, W] batch (mean over channels)."""
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError("expected two [B, C, H, W] tensors of one shape")
    if min(pred.shape[-2:]) < VIF_MIN_SIZE:
        raise ValueError(f"VIF needs images of at least {VIF_MIN_SIZE} x {VIF_MIN_SIZE} pixels, got {tuple(pred.shape[-2:])}")
    eps = 1e-10
    B, C = pred.shape[:2]
    p = pred.double().reshape(B * C, 1, *pred.shape[2:])
    t = target.double().reshape(B * C, 1, *target.shape[2:])
    num = torch.zeros(B * C, dtype=torch.float64, device=p.device)
    den = torch.zeros(B * C, dtype=torch.float64, device=p.device)
    for scale in range(4):
        n = 2 ** (4 - scale) + 1
        k = _gaussian_kernel2d(n, n / 5.0, p.device, p.dtype)[None, None]
        if scale > 0:
            t = F.conv2d(t, k)[:, :, ::2, ::2]
            p = F.conv2d(p, k)[:, :, ::2, ::2]
        mu_t, mu_p = F.conv2d(t, k), F.conv2d(p, k)
        s_tt = (F.conv2d(t * t, k) - mu_t * mu_t).clamp(min=0.0)
        s_pp = (F.conv2d(p * p, k) - mu_p * mu_p).clamp(min=0.0)
        s_tp = F.conv2d(t * p, k) - mu_t * mu_p
        g = s_tp / (s_tt + eps)
        s_v = s_pp - g * s_tp
        m = s_tt < eps
        g = torch.where(m, torch.zeros_like(g), g)
        s_v = torch.where(m, s_pp, s_v)
        s_tt = torch.where(m, torch.zeros_like(s_tt), s_tt)
        m = s_pp < eps
        g = torch.where(m, torch.zeros_like(g), g)
        s_v = torch.where(m, torch.zeros_like(s_v), s_v)
        m = g < 0
        s_v = torch.where(m, s_pp, s_v)
        g = torch.where(m, torch.zeros_like(g), g)
        s_v = s_v.clamp(min=eps)
        num = num + torch.log10(1.0 + g * g * s_tt / (s_v + sigma_n_sq)).sum(dim=(1, 2, 3))
        den = den + torch.log10(1.0 + s_tt / sigma_n_sq).sum(dim=(1, 2, 3))
    return (num / den).reshape(B, C).mean(dim=1)


class VIF:
    def __init__(self, sigma_n_sq: float = 2.0):
        self.sigma_n_sq = float(sigma_n_sq)
        self.reset()

    def reset(self) -> None:
        self.total = 0.0
        self.n = 0

    def update(self, pred: Tensor, target: Tensor) -> None:
        v = vif_per_image(pred, target, self.sigma_n_sq)
        self.total += float(v.sum())
        self.n += v.numel()

    def compute(self) -> float:
        return self.total / self.n if self.n else float("nan")


# {off, kr, kg, kb} of a luma standard: the divisions as ultrazoom_amd/csrc/mz_color.h writes them
LUMA_COEFFS = {"bt601": (16.0 / 255.0, 65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0), "full": (0.0, 0.299, 0.587, 0.114)}


def _check_luma(luma) -> None:
    if luma is not None and luma not in MZ_LUMA_STANDARDS:
        raise ValueError(f"luma is None, 'bt601' (studio range) or 'full' (full range), got {luma!r}")


def luma_plane(x: Tensor, standard: str = "bt601") -> Tensor:
    """The float64 Y plane [B, 1, H, W] of a [B, 3, H, W] tensor (R, G, B): off + kr R + kg G + kb B, added in this order, in plain torch
    arithmetic wherever the tensor lives (a product is rounded before it is added: the kernels fuse the two, which moves Y by at most
    three roundings of 2^-54).  A uint8 value v means v / 255."""
    luma_standard(standard)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected a [B, 3, H, W] tensor, got {tuple(x.shape)}")
    off, kr, kg, kb = LUMA_COEFFS[standard]
    v = x.double() / 255 if x.dtype == torch.uint8 else x.double()
    y = off + kr * v[:, 0:1]
    y = y + kg * v[:, 1:2]
    return y + kb * v[:, 2:3]


def _measured(img: Tensor, luma, shave: int) -> Tensor:
    """what the torch backend's meters see of an image: the shaved view, its Y plane with `luma`"""
    from .metrics import shaved

    img = shaved(img, shave)
    return img if luma is None else luma_plane(img, luma)


class TorchMeters:
    """The three meters above behind the `update(pred, target)` / `compute()` of `metrics.MetricsAccumulator`, with its `luma` and
    `shave`; VIF takes the updates whose measured images still have 41 x 41 pixels."""

    def __init__(self, luma: Optional[str] = None, shave: int = 0):
        self.luma, self.shave = luma, shave
        self.psnr, self.ssim, self.vif = PSNR(1.0), SSIM(), VIF()

    def update(self, pred: Tensor, target: Tensor) -> None:
        target, pred = _measured(target, self.luma, self.shave), _measured(pred, self.luma, self.shave)
        self.psnr.update(pred, target)
        self.ssim.update(pred, target)
        if min(target.shape[-2:]) >= VIF_MIN_SIZE:
            self.vif.update(pred, target)

    def compute(self) -> dict:
        return {"psnr": self.psnr.compute(), "ssim": self.ssim.compute(), "vif": self.vif.compute() if self.vif.n else None}


def _meters(backend: str, luma, shave: int):
    if backend == "hip":
        from .metrics import MetricsAccumulator

        return MetricsAccumulator(1.0, luma=luma, shave=shave)
    return TorchMeters(luma, shave)


def _evaluate(batches, step, backend: str, baseline: bool, luma, shave: int, extra_key: Optional[str] = None) -> dict:
    """The one loop.  step(batch, images so far) -> (input, prediction, target, per-batch differences or None).  The meters of `backend`
    take prediction and target; with `baseline` a second set takes the bicubic enlargement of the input.  With `extra_key` the mean square
    of all the differences becomes that key of the result: summed on the device and read in the meters' one read, after the loop."""
    meters, base = _meters(backend, luma, shave), _meters(backend, luma, shave) if baseline else None
    sq, count, n = None, 0, 0
    for batch in batches:
        x, pred, target, d = step(batch, n)
        meters.update(pred, target)
        if baseline:
            base.update(bicubic_baseline(x, target.shape[-2:], backend), target)
        if d is not None:
            sq = (d * d).sum() if sq is None else sq + (d * d).sum()
            count += d.numel()
        n += x.shape[0]
    if extra_key is None:
        res = meters.compute()
    elif sq is None:
        res = {**meters.compute(), extra_key: float("nan")}
    else:
        res, (total,) = meters.compute(extra=sq.reshape(1))
        res[extra_key] = total / count
    res["images"] = n
    return {**res, **{"bicubic_" + k: v for k, v in base.compute().items()}} if baseline else res  # (a second read, still after the loop)


def bicubic_baseline(x: Tensor, size, backend: str = "torch") -> Tensor:
    """The baseline the reference's validate.py:84-118 measures next to every result: `x` enlarged to `size` = (H, W) with plain bicubic
    interpolation (A = -0.75, no antialiasing: the model's own skip connection), clamped to [0, 1].  `backend="torch"`: `F.interpolate`
    wherever the tensor lives, in float64 like every computation of this file, rounded once to x's dtype (uint8: v / 255 in, clamp ->
    * 255 + 0.5 -> truncate out) -- the checker of the kernel; `backend="hip"`: the library's kernel (`ultrazoom_amd.interpolate`, CUDA
    tensors only), which accumulates in float64 and rounds once, too."""
    size = tuple(int(v) for v in size)
    if backend == "hip":
        from .interpolate import interpolate

        return interpolate(x, size=size, mode="bicubic", clamp=True)
    u8 = x.dtype == torch.uint8
    y = F.interpolate(x.double() / 255 if u8 else x.double(), size=size, mode="bicubic", align_corners=False).clamp(0, 1)
    return torch.floor(y * 255 + 0.5).to(torch.uint8) if u8 else y.to(x.dtype)


@torch.inference_mode()
def evaluate(model, pairs: Iterable[Tuple[Tensor, Tensor]], backend: str = "torch", ensemble: int = 1, baseline: bool = False,
             luma: Optional[str] = None, shave: int = 0) -> dict:
    """`pairs` yields (low-resolution input, high-resolution target) batches already on the model's device/dtype;
    returns {"psnr": ..., "ssim": ..., "vif": ..., "images": n} as the reference's test loop accumulates them (pretrain.py:301-329;
    "vif" is None when the images are smaller than the 41 x 41 pixels the metric needs).  `backend="torch"`: the functions above,
    wherever the tensors live; `backend="hip"`: the same metrics from the library's kernels (`ultrazoom_amd.metrics`, CUDA tensors
    only), accumulated on the device and read once at the end.  `ensemble` = 2, 4 or 8: the predictions are the self-ensemble of that
    many orientations (`ultrazoom_amd.ensemble.upscale_ensemble`, CUDA tensors only); 1 is the plain `model.upscale`.  `baseline=True`:
    the result also holds "bicubic_psnr", "bicubic_ssim" and "bicubic_vif", the same metrics of `bicubic_baseline(x, y's size, backend)`
    against y, accumulated beside the others (on the device with `backend="hip"`: nothing is read inside the loop).  `luma`, `shave`:
    every metric, the "bicubic_*" ones included, is taken on the Y plane and without `shave` border pixels (the module's docstring);
    the keys of the result are the same, and "vif" is None when fewer than 41 x 41 pixels are left."""
    if backend not in ("torch", "hip"):
        raise ValueError(f"backend is 'torch' or 'hip', got {backend!r}")
    _check_luma(luma)
    predict = model.upscale
    if ensemble != 1:
        from .ensemble import ORIENTATIONS, upscale_ensemble

        if ensemble not in ORIENTATIONS:
            raise ValueError(f"ensemble is 1, 2, 4 or 8 orientations, got {ensemble!r}")

        def predict(x):
            return upscale_ensemble(model, x, n=ensemble)

    def step(pair, n):
        x, y = pair
        return x, predict(x), y, None

    return _evaluate(pairs, step, backend, baseline, luma, shave)


@torch.inference_mode()
def lr_from_hr(hr: Tensor, ratio: int, filter: str = "bicubic", backend: str = "torch") -> Tuple[Tensor, Tensor]:
    """The low-resolution input of a high-resolution batch, as the reference derives it (data.py:91-108: an antialiased `Resize`,
    BICUBIC or BILINEAR; pretrain.py:301-329 validates on such pairs): `hr` [B, C, H, W] is cropped at the top-left to multiples of
    `ratio` (a view, nothing is copied) and resized by 1 / ratio.  Returns (lr, hr_cropped).  `backend="torch"`:
    `F.interpolate(..., antialias=True)` wherever the tensor lives (uint8 is not taken); `backend="hip"`: the library's kernel
    (`ultrazoom_amd.resize`, CUDA tensors only), which reads the cropped view in place.  The rest of the reference's degradation chain
    (blur, noise, JPEG: transforms.py) is `ultrazoom_amd.degrade`: `Degradation.apply` runs this resize between them."""
    if backend not in ("torch", "hip"):
        raise ValueError(f"backend is 'torch' or 'hip', got {backend!r}")
    resize_filter(filter)
    ratio = int(ratio)
    if hr.dim() != 4 or ratio < 1 or hr.shape[-2] < ratio or hr.shape[-1] < ratio:
        raise ValueError(f"expected a [B, C, H, W] tensor of at least {ratio} x {ratio} pixels, got {tuple(hr.shape)}")
    h, w = hr.shape[-2] // ratio, hr.shape[-1] // ratio
    hr = hr[..., : h * ratio, : w * ratio]
    if backend == "hip":
        from .resize import resize

        return resize(hr, (h, w), filter=filter), hr
    return F.interpolate(hr, size=(h, w), mode=filter, antialias=True, align_corners=False), hr


def evaluate_hr(model, hr_batches: Iterable[Tensor], *, filter: str = "bicubic", backend: str = "torch", degrade=None,
                ensemble: int = 1, baseline: bool = False, luma: Optional[str] = None, shave: int = 0) -> dict:
    """`evaluate` on high-resolution batches alone: each is turned into its (LR, HR) pair by `lr_from_hr` at the model's ratio.  With
    `backend="hip"` the chain HR -> LR -> upscale -> metrics stays on the device and is read once, at the end.

    `degrade`: a `ultrazoom_amd.degrade.Degradation` (`backend="hip"` only; its own `filter` is used) validates under the reference's
    blind-degradation recipe instead: the pairs come from `Degradation.apply` (blur -> noise -> resize -> JPEG, image n of the run
    drawing parameters and noise n of the seed), the network runs once per batch for the clamped SR and the quality head's output,
    and the result gains "deg_l2": the mean squared error of that output against the normalised parameters (pretrain.py:246-250),
    accumulated on the device and read with the image metrics.

    `ensemble` as for `evaluate`; with `degrade` the clamped SR is the self-ensemble and the quality head still runs once, on the
    degraded input as it is.

    `baseline` as for `evaluate`: the "bicubic_*" metrics of the low-resolution input (with `degrade`: the degraded one) enlarged to the
    target's size with plain bicubic interpolation.

    `luma`, `shave` as for `evaluate` (the usual protocol: `luma="bt601", shave=model.upscale_ratio`), with `degrade` too; "deg_l2" does
    not depend on them."""
    _check_luma(luma)
    if degrade is None:
        return evaluate(model, (lr_from_hr(hr, model.upscale_ratio, filter, backend) for hr in hr_batches), backend, ensemble, baseline,
                        luma, shave)
    if backend != "hip":
        raise ValueError("degrade runs on the device only: use backend='hip'. There is no CPU path.")
    from .ensemble import ORIENTATIONS

    if ensemble not in ORIENTATIONS:
        raise ValueError(f"ensemble is 1, 2, 4 or 8 orientations, got {ensemble}")
    return _evaluate_degraded(model, hr_batches, degrade, int(ensemble), bool(baseline), luma, shave)


@torch.inference_mode()
def _evaluate_degraded(model, hr_batches: Iterable[Tensor], degrade, ensemble: int = 1, baseline: bool = False, luma: Optional[str] = None,
                       shave: int = 0) -> dict:
    def step(hr, n):
        lr, target, want = degrade.apply(hr, model.upscale_ratio, index=n)
        if ensemble == 1:
            sr, qa = model.forward(lr)
            sr = sr.clamp(0, 1)
        else:
            from .ensemble import upscale_ensemble

            qa = model.predict_degredation(lr)
            sr = upscale_ensemble(model, lr, n=ensemble)
        return lr, sr, target, qa.double() - want.double()

    return _evaluate(hr_batches, step, "hip", baseline, luma, shave, extra_key="deg_l2")
