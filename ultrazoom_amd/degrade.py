"""The reference's degradation chain on the MI355X: `mz_blur`, `mz_noise`, `mz_jpeg` (include/mewzoom_hip.h) behind a tensor interface,
and `Degradation`, the blind-degradation recipe of the reference's data loader (data.py:134-164, transforms.py): blur -> noise ->
antialiased resize -> JPEG, whose three parameters, normalised to [0, 1], are the target of the quality head (pretrain.py:246-250).

The arithmetic (ultrazoom_amd/csrc/mz_degrade.h states it in full) runs in HIP on the tensors as they lie in memory: any strides,
float32 / bfloat16 / float16 / uint8 (a uint8 value v means v / 255 and is stored as clamp -> * 255 + 0.5 -> truncate).  Nothing is
copied and nothing here synchronises with the host.  torch's generator cannot be matched on the device, so the noise and the sampled
parameters come from the library's own stream: Philox4x32-10 keyed by a seed, reproducible from the seed alone."""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _ffi

_M64 = 2**64 - 1
BLUR_MAX_HALF = 15  # int(3 sigma) beyond this is refused (include/mewzoom_hip.h)
PARAMETER_STREAM = _M64  # the stream id `Degradation.sample` draws from; noise uses stream ids offset + b


def _per_image(value, B: int, name: str) -> Optional[list]:
    """None for a scalar; the list of B values for a sequence"""
    if isinstance(value, Tensor):
        value = value.tolist()
    if isinstance(value, (int, float)):
        return None
    value = list(value)
    if len(value) != B:
        raise ValueError(f"{name} is a scalar or a sequence of one value per image ({B}), got {len(value)} values")
    return value


def _run(x: Tensor, out: Tensor, values, call) -> None:
    """call(x view, out view, images, value, image index of the first) once for the batch, or once per image"""
    if values is None:
        call(x, out, x.shape[0], None, 0)
    else:
        for b, v in enumerate(values):
            call(x[b:b + 1], out[b:b + 1], 1, v, b)


def gaussian_blur(x: Tensor, sigma: Union[float, Sequence[float]], out: Optional[Tensor] = None) -> Tensor:
    """torchvision's `gaussian_blur(x, 2 * int(3 * sigma) + 1, [sigma, sigma])` as transforms.py:36-43 calls it, of a logical
    [B, 3, H, W] CUDA tensor: reflect padding, weights and both passes in float64.  `sigma` is a scalar or one value per image (one
    call per image on a view of it).  Returns a new dense tensor of x's dtype, or `out` (any strides).  sigma < 1 / 3 copies;
    int(3 sigma) must stay below min(H, W) and at most 15.  x and out must not overlap."""
    elem, B, H, W = _ffi.check_image_batch(x, "gaussian_blur", out)
    sigmas = _per_image(sigma, B, "sigma")
    for s in ([sigma] if sigmas is None else sigmas):
        s = float(s)
        if not (0.0 <= s and int(3 * s) <= BLUR_MAX_HALF):
            raise ValueError(f"sigma {s}: need 0 <= sigma and int(3 sigma) <= {BLUR_MAX_HALF}")
        if int(3 * s) >= min(H, W):
            raise ValueError(f"sigma {s} needs {int(3 * s)} pixels of reflect padding: a {H} x {W} image is too small")
    with _ffi.image_frame(x, out, x.shape) as (out, _, stream):
        _run(x, out, sigmas, lambda xv, ov, n, s, b: _ffi.blur(*_ffi.pair(xv), *_ffi.pair(ov), elem, n, H, W, float(sigma if s is None else s),
                                                              stream))
    return out


def gaussian_noise(x: Tensor, sigma: Union[float, Sequence[float]], *, seed: int, offset: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """torchvision's `gaussian_noise(x, mean=0, sigma=sigma, clip=True)` on the [0, 1] scale: clamp(x + sigma n, 0, 1) in float64, n from
    the library's Philox stream: image b of the call draws from stream `offset + b` of `seed`, element by element, so a batch split
    into calls (image b with offset + b) gives the bits of the one call.  `out=x` works in place."""
    elem, B, H, W = _ffi.check_image_batch(x, "gaussian_noise", out)
    sigmas = _per_image(sigma, B, "sigma")
    for s in ([sigma] if sigmas is None else sigmas):
        if not 0.0 <= float(s) <= 1e6:
            raise ValueError(f"sigma {s}: need 0 <= sigma <= 1e6")
    with _ffi.image_frame(x, out, x.shape) as (out, _, stream):
        _run(x, out, sigmas, lambda xv, ov, n, s, b: _ffi.noise(*_ffi.pair(xv), *_ffi.pair(ov), elem, n, H, W, float(sigma if s is None else s),
                                                               seed, int(offset) + b, stream))
    return out


def jpeg(x: Tensor, quality: Union[int, Sequence[int]], out: Optional[Tensor] = None) -> Tensor:
    """A baseline JPEG round trip (4:2:0, the Annex K tables scaled by `quality` 1..100) of a logical [B, 3, H, W] CUDA tensor, modelled in
    arithmetic on the device: what torchvision's `jpeg(x, quality)` does through a codec, without one.  `quality` is a scalar or one
    value per image.  x and out must not overlap."""
    elem, B, H, W = _ffi.check_image_batch(x, "jpeg", out)
    qualities = _per_image(quality, B, "quality")
    for q in ([quality] if qualities is None else qualities):
        if int(q) != q or not 1 <= int(q) <= 100:
            raise ValueError(f"quality is an integer in 1..100, got {q!r}")
    # calls on one stream run one after the other: one workspace serves all
    with _ffi.image_frame(x, out, x.shape, lambda: _ffi.jpeg_workspace_bytes(B if qualities is None else 1, H, W)) as (out, ws, stream):
        _run(x, out, qualities, lambda xv, ov, n, q, b: _ffi.jpeg(*_ffi.pair(xv), *_ffi.pair(ov), elem, n, H, W,
                                                                 int(quality if q is None else q), *ws, stream))
    return out


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> List[int]:
    """One block of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) on the host: the generator
    of ultrazoom_amd/csrc/mz_degrade.h, restated in Python integers."""
    c0, c1, c2, c3 = (int(v) & 0xFFFFFFFF for v in counter)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


@dataclass(frozen=True)
class Degradation:
    """The blind-degradation recipe of the reference's data loader with its default ranges (data.py:24-32): per image a Gaussian blur
    sigma, a Gaussian noise sigma and a JPEG compression drawn uniformly from the ranges, applied as blur -> noise -> antialiased
    resize by 1 / ratio -> JPEG at quality int(100 (1 - compression)).  `filter` is "bicubic" or "bilinear" (the reference also draws
    NEAREST, which the resampling kernel does not offer).  Everything random follows from `seed` and the image's index in the run."""

    blur: Tuple[float, float] = (0.0, 1.0)
    noise: Tuple[float, float] = (0.0, 0.1)
    compression: Tuple[float, float] = (0.0, 0.8)
    filter: str = "bicubic"
    seed: int = 0

    def __post_init__(self):
        _ffi.resize_filter(self.filter)
        for name in ("blur", "noise", "compression"):
            lo, hi = getattr(self, name)
            if not 0.0 <= lo < hi:
                raise ValueError(f"{name} is a range (min, max) with 0 <= min < max, got {(lo, hi)}")
        if self.compression[1] > 0.99:
            raise ValueError(f"compression is at most 0.99 (quality 1), got {self.compression}")

    def sample(self, B: int, index: int = 0) -> List[Tuple[float, float, float]]:
        """(blur sigma, noise sigma, compression) of images index .. index + B - 1 of a run, on the host: image g takes the first three
        words u of the Philox block with key `seed` and counter (g, stream id 2^64 - 1); value = min + (max - min) (u + 0.5) / 2^32."""
        key = (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)
        rows = []
        for g in range(int(index), int(index) + int(B)):
            u = philox4x32_10((g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, PARAMETER_STREAM & 0xFFFFFFFF, PARAMETER_STREAM >> 32), key)
            rows.append(tuple(lo + (hi - lo) * ((u[k] + 0.5) / 4294967296.0)
                              for k, (lo, hi) in enumerate((self.blur, self.noise, self.compression))))
        return rows

    def targets(self, params: Sequence[Tuple[float, float, float]]) -> List[List[float]]:
        """(value - min) / (max - min) of each parameter (data.py:150-162): the quality head's target"""
        ranges = (self.blur, self.noise, self.compression)
        return [[(v - lo) / (hi - lo) for v, (lo, hi) in zip(row, ranges)] for row in params]

    @torch.inference_mode()
    def apply(self, hr: Tensor, ratio: int, index: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
        """(lr, hr_cropped, targets) of a high-resolution CUDA batch whose first image is image `index` of the run: `hr` cropped at the
        top-left to multiples of `ratio` (a view), its degraded low-resolution counterpart [B, 3, H / ratio, W / ratio] of hr's dtype,
        and the normalised parameters as a float32 [B, 3] tensor on hr's device.  The noise of image b is stream index + b of `seed`."""
        from .evaluate import lr_from_hr

        _, B, H, W = _ffi.check_image_batch(hr, "Degradation.apply")
        ratio = int(ratio)
        if ratio < 1 or H < ratio or W < ratio:
            raise ValueError(f"expected a [B, 3, H, W] tensor of at least {ratio} x {ratio} pixels, got {tuple(hr.shape)}")
        params = self.sample(B, index)
        h, w = H // ratio, W // ratio
        cropped = hr[..., : h * ratio, : w * ratio]
        x = gaussian_blur(cropped, [p[0] for p in params])
        gaussian_noise(x, [p[1] for p in params], seed=self.seed, offset=index, out=x)
        lr, _ = lr_from_hr(x, ratio, filter=self.filter, backend="hip")
        lr = jpeg(lr, [int(100 * (1 - p[2])) for p in params])
        targets = torch.tensor(self.targets(params), dtype=torch.float32).to(hr.device, non_blocking=True)
        return lr, cropped, targets
