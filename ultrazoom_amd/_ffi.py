"""ctypes binding of libmewzoom_hip.so (include/mewzoom_hip.h).

There is deliberately no fallback: if the shared library is missing or a call fails, an exception
is raised.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or
``ultrazoom_amd/csrc/build.sh``).
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p
from pathlib import Path

LIB_NAME = "libmewzoom_hip.so"
LIB_PATH = Path(__file__).resolve().parent / LIB_NAME

MZ_F32, MZ_BF16, MZ_F16 = 0, 1, 2

MZ_ERR_INVALID_ARGUMENT = -1
MZ_ERR_WORKSPACE_TOO_SMALL = -5

MZ_METRIC_SLOTS = 16  # doubles per image of mz_metrics' output (include/mewzoom_hip.h documents the slots)
MZ_METRIC_PSNR, MZ_METRIC_SSIM, MZ_METRIC_VIF = 1, 2, 4
MZ_RESIZE_BICUBIC, MZ_RESIZE_BILINEAR = 0, 1
MZ_RESIZE_MAX_TAPS = 66  # taps of one output at the largest accepted ratio (n_in / n_out = 16, bicubic)
MZ_INTERP_NEAREST, MZ_INTERP_BILINEAR, MZ_INTERP_BICUBIC = 0, 1, 2
MZ_LUMA_STANDARDS = {"bt601": 0, "full": 1}  # studio range (MATLAB rgb2ycbcr, basicsr) / full range (JFIF, Pillow's "L")


class MzConfig(Structure):
    _fields_ = [
        ("upscale_ratio", c_int32),
        ("primary_channels", c_int32),
        ("primary_layers", c_int32),
        ("secondary_channels", c_int32),
        ("secondary_layers", c_int32),
        ("tertiary_channels", c_int32),
        ("tertiary_layers", c_int32),
        ("quaternary_channels", c_int32),
        ("quaternary_layers", c_int32),
        ("hidden_ratio", c_int32),
        ("num_deg_features", c_int32),
    ]


class MzImageView(Structure):
    """mz_image_view: the address of element (image 0, channel 0, row 0, column 0) and four signed element strides."""

    _fields_ = [("data", c_void_p), ("stride", c_int64 * 4)]


class MzDebugStep(Structure):
    """mz_debug_step: one step of a forward pass (include/mewzoom_hip.h documents the fields)."""

    _fields_ = [(name, c_int32) for name in "kind op cin cout B H W Hout Wout fused".split()] + [
        ("off", c_int64 * 3), ("bytes", c_uint64 * 3), ("kernel", c_char_p)]


class MewZoomHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libmewzoom_hip error {code}: {message}")
        self.code = code


_lib = None


def _declare(lib) -> None:
    H = c_void_p
    lib.mz_create.argtypes = [POINTER(MzConfig), c_int, POINTER(H)]
    lib.mz_destroy.argtypes = [H]
    lib.mz_num_weights.argtypes = [H]
    lib.mz_weight_info.argtypes = [H, c_int, POINTER(c_char_p), POINTER(c_int64)]
    lib.mz_set_weight.argtypes = [H, c_char_p, c_void_p, POINTER(c_int64), c_int, c_void_p]
    lib.mz_weights_complete.argtypes = [H]
    lib.mz_workspace_bytes.argtypes = [H, c_int, c_int, c_int, c_int, POINTER(c_size_t)]
    lib.mz_forward.argtypes = [H, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]
    lib.mz_forward_u8.argtypes = [H, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]
    lib.mz_forward_u8.restype = c_int
    lib.mz_forward_view.argtypes = [H, POINTER(MzImageView), POINTER(MzImageView), c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    POINTER(c_int32), c_void_p, c_size_t, c_int, c_void_p]
    lib.mz_forward_view.restype = c_int
    lib.mz_metrics_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_size_t)]
    lib.mz_metrics_workspace_bytes.restype = c_int
    lib.mz_metrics.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                               c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mz_metrics.restype = c_int
    lib.mz_luma.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.mz_luma.restype = c_int
    lib.mz_metrics_luma_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_size_t)]
    lib.mz_metrics_luma_workspace_bytes.restype = c_int
    lib.mz_metrics_luma.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                                    c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mz_metrics_luma.restype = c_int
    lib.mz_debug_luma_coeffs.argtypes = [c_int, POINTER(c_double)]
    lib.mz_debug_luma_coeffs.restype = c_int
    lib.mz_resize_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]
    lib.mz_resize_workspace_bytes.restype = c_int
    lib.mz_resize.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                              POINTER(c_int32), c_void_p, c_size_t, c_void_p]
    lib.mz_resize.restype = c_int
    lib.mz_debug_resize_taps.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_double), c_int]
    lib.mz_debug_resize_taps.restype = c_int
    lib.mz_interpolate.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                   POINTER(c_int32), c_void_p]
    lib.mz_interpolate.restype = c_int
    lib.mz_debug_interp_taps.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_double)]
    lib.mz_debug_interp_taps.restype = c_int
    lib.mz_blur.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_double, c_void_p]
    lib.mz_blur.restype = c_int
    lib.mz_noise.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_double, c_uint64, c_uint64, c_void_p]
    lib.mz_noise.restype = c_int
    lib.mz_jpeg_workspace_bytes.argtypes = [c_int, c_int, c_int, POINTER(c_size_t)]
    lib.mz_jpeg_workspace_bytes.restype = c_int
    lib.mz_jpeg.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]
    lib.mz_jpeg.restype = c_int
    lib.mz_debug_blur_weights.argtypes = [c_double, POINTER(c_double), c_int]
    lib.mz_debug_blur_weights.restype = c_int
    lib.mz_debug_jpeg_qtable.argtypes = [c_int, POINTER(c_uint8), POINTER(c_uint8)]
    lib.mz_debug_jpeg_qtable.restype = c_int
    lib.mz_debug_philox.argtypes = [POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]
    lib.mz_debug_philox.restype = c_int
    lib.mz_dihedral_inverse.argtypes = [c_int]
    lib.mz_dihedral_inverse.restype = c_int
    lib.mz_dihedral.argtypes = [POINTER(MzImageView), POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.mz_dihedral.restype = c_int
    lib.mz_ensemble_workspace_bytes.argtypes = [c_int, c_int, c_int, POINTER(c_size_t)]
    lib.mz_ensemble_workspace_bytes.restype = c_int
    lib.mz_ensemble_add.argtypes = [POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]
    lib.mz_ensemble_add.restype = c_int
    lib.mz_ensemble_finish.argtypes = [POINTER(MzImageView), c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int32), c_void_p, c_size_t,
                                       c_void_p]
    lib.mz_ensemble_finish.restype = c_int
    lib.mz_padded_channels.argtypes = [c_int]
    lib.mz_op_conv.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p] + [c_int] * 8 + [c_void_p]
    lib.mz_op_conv_film.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]
    lib.mz_op_conv_film.restype = c_int
    lib.mz_op_conv_mix.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p] + [c_int] * 5 + [c_void_p]
    lib.mz_op_conv_mix.restype = c_int
    lib.mz_op_stem.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]
    lib.mz_op_final.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]
    lib.mz_last_error.restype = c_char_p
    lib.mz_version.restype = c_char_p
    lib.mz_flops_per_image.argtypes = [H, c_int, c_int]
    lib.mz_flops_per_image.restype = c_double
    lib.mz_debug_schedule.argtypes = [H, c_int, c_int, c_int, c_int, c_int, POINTER(MzDebugStep), c_int]
    lib.mz_debug_schedule.restype = c_int
    lib.mz_profile_enable.argtypes = [H, c_int]
    lib.mz_profile_read.argtypes = [H] + [POINTER(c_double)] * 5
    lib.mz_profile_dump.argtypes = [H, c_char_p]
    lib.mz_profile_dump.restype = c_int
    for name in (
        "mz_create mz_destroy mz_num_weights mz_weight_info mz_set_weight mz_weights_complete mz_workspace_bytes "
        "mz_forward mz_padded_channels mz_op_conv mz_op_stem mz_op_final mz_profile_enable mz_profile_read"
    ).split():
        getattr(lib, name).restype = c_int


def lib():
    """The loaded shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("MEWZOOM_HIP_LIB", LIB_PATH))
        if not path.exists():
            raise ImportError(
                f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` from the repository root. There is no fallback path."
            )
        _lib = ctypes.CDLL(str(path))
        _declare(_lib)
    return _lib


def check(code: int) -> None:
    if code != 0:
        raise MewZoomHipError(code, lib().mz_last_error().decode())


def dtype_code(torch_dtype) -> int:
    import torch

    table = {torch.float32: MZ_F32, torch.bfloat16: MZ_BF16, torch.float16: MZ_F16}
    if torch_dtype not in table:
        raise TypeError(f"unsupported dtype {torch_dtype}; use float32, bfloat16 or float16")
    return table[torch_dtype]


def elem_code(torch_dtype) -> int:
    """The `elem` of the image-view entries: 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8 (mz_forward_view: 0 = the handle's dtype, 1 = uint8)."""
    import torch

    ELEM = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.uint8: 3}
    if torch_dtype not in ELEM:
        raise TypeError(f"unsupported dtype {torch_dtype}; use float32, bfloat16, float16 or uint8")
    return ELEM[torch_dtype]


def check_same_batch(x, other, shape, names=("x", "out")) -> None:
    """`other` (the output of `x`, or a second input) is on x's device, of x's dtype and of `shape`."""
    if other.device != x.device:
        raise RuntimeError(f"{names[0]} is on {x.device} but {names[1]} is on {other.device}")
    if other.dtype != x.dtype:
        raise TypeError(f"{names[0]} ({x.dtype}) and {names[1]} ({other.dtype}) should have the same dtype")
    if tuple(other.shape) != tuple(shape):
        raise ValueError(f"{names[1]} has shape {tuple(other.shape)}, expected the one shape {tuple(shape)}")


def check_image_batch(x, what: str, other=None, names=("x", "out")):
    """(elem code, B, H, W) of a logical [B, 3, H, W] CUDA image batch given to ultrazoom_amd.`what`; `other` as check_same_batch."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected a [B, 3, H, W] tensor, got {tuple(x.shape)}")
    elem = elem_code(x.dtype)
    if not x.is_cuda:
        raise RuntimeError(f"ultrazoom_amd.{what} computes on an MI355X only: move the image to a 'cuda' device. There is no CPU path.")
    B, _, H, W = x.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"an empty batch or image: {tuple(x.shape)}")
    if other is not None:
        check_same_batch(x, other, x.shape, names)
    return elem, B, H, W


def output_shape(B: int, size, window, size_check=None):
    """(Hout, Wout, window as a tuple or None, the shape `out` must have) of a call that resamples B images to `size` = (Hout, Wout) and
    stores `window` = (y0, x0, h, w) of the result, or all of it; size_check(Hout, Wout), an entry's own bound on the size, runs between
    the two."""
    size = tuple(int(v) for v in size)
    if len(size) != 2 or min(size) < 1:
        raise ValueError(f"size is (Hout, Wout) with both at least 1, got {size}")
    Hout, Wout = size
    if size_check is not None:
        size_check(Hout, Wout)
    if window is None:
        return Hout, Wout, None, (B, 3, Hout, Wout)
    window = tuple(int(v) for v in window)
    if len(window) != 4:
        raise ValueError("window is (y0, x0, h, w) in output pixels")
    y0, x0, h, w = window
    if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > Hout or x0 + w > Wout:
        raise ValueError(f"window {window} is empty or not inside the {Hout} x {Wout} result")
    return Hout, Wout, window, (B, 3, h, w)


def view(ptr, strides) -> MzImageView:
    """An mz_image_view: the address of element (0, 0, 0, 0) and the element strides (image, channel, row, column; signed)."""
    return MzImageView(c_void_p(ptr), (c_int64 * 4)(*[int(v) for v in strides]))


def _window_arg(window):
    """`window` = (y0, x0, h, w) or None as the `const int32_t window[4]` of an entry."""
    return (c_int32 * 4)(*[int(v) for v in window]) if window is not None else None


def make_config(cfg: dict) -> MzConfig:
    return MzConfig(**{k: int(cfg[k]) for k, _ in MzConfig._fields_})


def metrics_workspace_bytes(B: int, H: int, W: int, which: int) -> int:
    out = c_size_t()
    check(lib().mz_metrics_workspace_bytes(B, H, W, which, byref(out)))
    return int(out.value)


def metrics(pred_ptr, pred_strides, target_ptr, target_strides, elem, B, H, W, which, data_range, sigma_n_sq, out_ptr, ws_ptr, ws_bytes,
            stream) -> None:
    """mz_metrics: the two views as for Handle.forward_view; `elem` 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8."""
    pv, tv = view(pred_ptr, pred_strides), view(target_ptr, target_strides)
    check(
        lib().mz_metrics(
            byref(pv), byref(tv), int(elem), B, H, W, int(which), float(data_range), float(sigma_n_sq), c_void_p(out_ptr),
            c_void_p(ws_ptr), ws_bytes, c_void_p(stream),
        )
    )


def luma_standard(standard) -> int:
    """The `standard` code of the luma entries: "bt601" -> 0, "full" -> 1."""
    if standard not in MZ_LUMA_STANDARDS:
        raise ValueError(f"luma standard is 'bt601' (studio range) or 'full' (full range), got {standard!r}")
    return MZ_LUMA_STANDARDS[standard]


def luma(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, standard, clamp, stream) -> None:
    """mz_luma: x a view of [B,3,H,W], out a view of [B,1,H,W], as for `resize`; `standard` 0 bt601, 1 full; no workspace."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    check(lib().mz_luma(byref(xv), byref(ov), int(elem), B, H, W, int(standard), int(bool(clamp)), c_void_p(stream)))


def luma_coeffs(standard: int):
    """mz_debug_luma_coeffs (host only): [off, kr, kg, kb], the constants the kernels compile."""
    out = (c_double * 4)()
    check(lib().mz_debug_luma_coeffs(int(standard), out))
    return [float(v) for v in out]


def metrics_luma_workspace_bytes(B: int, H: int, W: int, which: int) -> int:
    out = c_size_t()
    check(lib().mz_metrics_luma_workspace_bytes(B, H, W, which, byref(out)))
    return int(out.value)


def metrics_luma(pred_ptr, pred_strides, target_ptr, target_strides, elem, B, H, W, which, standard, data_range, sigma_n_sq, out_ptr, ws_ptr,
                 ws_bytes, stream) -> None:
    """mz_metrics_luma: `metrics` on the float64 Y planes of the two [B,3,H,W] views."""
    pv, tv = view(pred_ptr, pred_strides), view(target_ptr, target_strides)
    check(
        lib().mz_metrics_luma(
            byref(pv), byref(tv), int(elem), B, H, W, int(which), int(standard), float(data_range), float(sigma_n_sq), c_void_p(out_ptr),
            c_void_p(ws_ptr), ws_bytes, c_void_p(stream),
        )
    )


def resize_workspace_bytes(Hin: int, Win: int, Hout: int, Wout: int, filter_: int) -> int:
    out = c_size_t()
    check(lib().mz_resize_workspace_bytes(Hin, Win, Hout, Wout, int(filter_), byref(out)))
    return int(out.value)


def resize(x_ptr, x_strides, out_ptr, out_strides, elem, B, Hin, Win, Hout, Wout, filter_, clamp, window, ws_ptr, ws_bytes, stream) -> None:
    """mz_resize: the two views as for Handle.forward_view (out: of the window); `elem` 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8;
    `window` = (y0, x0, h, w) in pixels of the Hout x Wout result, or None."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    win = _window_arg(window)
    check(
        lib().mz_resize(
            byref(xv), byref(ov), int(elem), B, Hin, Win, Hout, Wout, int(filter_), int(bool(clamp)), win, c_void_p(ws_ptr), ws_bytes,
            c_void_p(stream),
        )
    )


def resize_taps(n_in: int, n_out: int, filter_: int, i: int):
    """mz_debug_resize_taps (host only): (first, [w_0 .. w_{count-1}]) of output index i of one axis."""
    first = c_int()
    w = (c_double * MZ_RESIZE_MAX_TAPS)()
    count = lib().mz_debug_resize_taps(n_in, n_out, int(filter_), i, byref(first), w, MZ_RESIZE_MAX_TAPS)
    if count < 0:
        check(count)
    return int(first.value), [float(w[j]) for j in range(count)]


def interpolate(x_ptr, x_strides, out_ptr, out_strides, elem, B, Hin, Win, Hout, Wout, mode, clamp, window, stream) -> None:
    """mz_interpolate: the two views and the window as for `resize`; `mode` 0 nearest, 1 bilinear, 2 bicubic (A = -0.75); no workspace."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    win = _window_arg(window)
    check(lib().mz_interpolate(byref(xv), byref(ov), int(elem), B, Hin, Win, Hout, Wout, int(mode), int(bool(clamp)), win, c_void_p(stream)))


def interp_taps(n_in: int, n_out: int, mode: int, i: int):
    """mz_debug_interp_taps (host only): ([idx_0 ..], [w_0 ..]) of output index i of one axis, 1, 2 or 4 taps."""
    idx, w = (c_int * 4)(), (c_double * 4)()
    count = lib().mz_debug_interp_taps(n_in, n_out, int(mode), i, idx, w)
    if count < 0:
        check(count)
    return [int(idx[j]) for j in range(count)], [float(w[j]) for j in range(count)]


def blur(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, sigma, stream) -> None:
    """mz_blur: the two views as for `resize`; `elem` 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    check(lib().mz_blur(byref(xv), byref(ov), int(elem), B, H, W, float(sigma), c_void_p(stream)))


def noise(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, sigma, seed, offset, stream) -> None:
    """mz_noise: `seed` and `offset` are taken modulo 2^64; out may be the same view as x."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    check(lib().mz_noise(byref(xv), byref(ov), int(elem), B, H, W, float(sigma), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                         c_void_p(stream)))


def jpeg_workspace_bytes(B: int, H: int, W: int) -> int:
    out = c_size_t()
    check(lib().mz_jpeg_workspace_bytes(B, H, W, byref(out)))
    return int(out.value)


def jpeg(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, quality, ws_ptr, ws_bytes, stream) -> None:
    """mz_jpeg: the round trip at `quality` 1..100 on a workspace of `jpeg_workspace_bytes(B, H, W)` bytes."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    check(lib().mz_jpeg(byref(xv), byref(ov), int(elem), B, H, W, int(quality), c_void_p(ws_ptr), ws_bytes, c_void_p(stream)))


def blur_weights(sigma: float):
    """mz_debug_blur_weights (host only): the k = 2 * int(3 sigma) + 1 normalised weights the kernel is handed."""
    w = (c_double * 31)()
    k = lib().mz_debug_blur_weights(float(sigma), w, 31)
    if k < 0:
        check(k)
    return [float(w[j]) for j in range(k)]


def jpeg_qtable(quality: int):
    """mz_debug_jpeg_qtable (host only): (luminance, chrominance), 64 integers each, row-major."""
    a, b = (c_uint8 * 64)(), (c_uint8 * 64)()
    check(lib().mz_debug_jpeg_qtable(int(quality), a, b))
    return list(a), list(b)


def philox(counter, key):
    """mz_debug_philox (host only): the four words of one Philox4x32-10 block, from the function the noise kernel compiles."""
    out = (c_uint32 * 4)()
    check(lib().mz_debug_philox((c_uint32 * 4)(*counter), (c_uint32 * 2)(*key), out))
    return [int(v) for v in out]


def dihedral_inverse(k: int) -> int:
    """mz_dihedral_inverse (host only): the orientation that undoes orientation k; negative outside 0..7."""
    return int(lib().mz_dihedral_inverse(int(k)))


def dihedral(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, k, stream) -> None:
    """mz_dihedral: out, a view of [B,3,H',W'], receives T(x, k) of the [B,3,H,W] view x; the views as for `resize`."""
    xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
    check(lib().mz_dihedral(byref(xv), byref(ov), int(elem), B, H, W, int(k), c_void_p(stream)))


def ensemble_workspace_bytes(B: int, H: int, W: int) -> int:
    out = c_size_t()
    check(lib().mz_ensemble_workspace_bytes(B, H, W, byref(out)))
    return int(out.value)


def ensemble_add(y_ptr, y_strides, elem, B, H, W, k, first, ws_ptr, ws_bytes, stream) -> None:
    """mz_ensemble_add: the pass result y, a view in ITS orientation ([B,3,W,H] when k & 4), turned back and stored in (`first`) or added
    to the float32 accumulator of the [B,3,H,W] result."""
    yv = view(y_ptr, y_strides)
    check(lib().mz_ensemble_add(byref(yv), int(elem), B, H, W, int(k), int(bool(first)), c_void_p(ws_ptr), ws_bytes, c_void_p(stream)))


def ensemble_finish(out_ptr, out_strides, elem, B, H, W, n, clamp, window, ws_ptr, ws_bytes, stream) -> None:
    """mz_ensemble_finish: the mean of the n results added, into out (a view of the window, as for `resize`)."""
    ov = view(out_ptr, out_strides)
    win = _window_arg(window)
    check(lib().mz_ensemble_finish(byref(ov), int(elem), B, H, W, int(n), int(bool(clamp)), win, c_void_p(ws_ptr), ws_bytes, c_void_p(stream)))


class Handle:
    """Owns one mz_handle."""

    def __init__(self, cfg: dict, dtype_code_: int):
        self._h = c_void_p()
        check(lib().mz_create(byref(make_config(cfg)), dtype_code_, byref(self._h)))
        self.dtype_code = dtype_code_

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None:
            _lib.mz_destroy(self._h)
            self._h = c_void_p()

    __del__ = close

    # A handle owns device memory through a raw pointer: copying the Python object would free it twice.
    def __copy__(self):
        raise TypeError("an mz_handle cannot be copied; build a new Handle")

    def __deepcopy__(self, memo):
        raise TypeError("an mz_handle cannot be copied; build a new Handle")

    def __reduce__(self):
        raise TypeError("an mz_handle cannot be pickled; build a new Handle")

    @property
    def ptr(self):
        return self._h

    def weight_infos(self):
        n = lib().mz_num_weights(self._h)
        out = []
        for i in range(n):
            name = c_char_p()
            shape = (c_int64 * 4)()
            ndim = lib().mz_weight_info(self._h, i, byref(name), shape)
            if ndim < 0:
                check(ndim)
            out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim))))
        return out

    def set_weight(self, name: str, dev_ptr: int, shape, stream: int) -> None:
        arr = (c_int64 * 4)(*list(shape) + [0] * (4 - len(shape)))
        check(lib().mz_set_weight(self._h, name.encode(), c_void_p(dev_ptr), arr, len(shape), c_void_p(stream)))

    def weights_complete(self) -> None:
        check(lib().mz_weights_complete(self._h))

    def workspace_bytes(self, B: int, H: int, W: int, max_in_flight: int = 0) -> int:
        out = c_size_t()
        check(lib().mz_workspace_bytes(self._h, B, H, W, max_in_flight, byref(out)))
        return int(out.value)

    def forward(self, x_ptr, sr_ptr, qa_ptr, B, H, W, clamp, ws_ptr, ws_bytes, max_in_flight, stream) -> None:
        check(
            lib().mz_forward(
                self._h, c_void_p(x_ptr), c_void_p(sr_ptr), c_void_p(qa_ptr) if qa_ptr else None, B, H, W, int(clamp),
                c_void_p(ws_ptr), ws_bytes, max_in_flight, c_void_p(stream),
            )
        )

    def forward_u8(self, x_ptr, sr_ptr, qa_ptr, B, H, W, ws_ptr, ws_bytes, max_in_flight, stream) -> None:
        check(
            lib().mz_forward_u8(
                self._h, c_void_p(x_ptr), c_void_p(sr_ptr), c_void_p(qa_ptr) if qa_ptr else None, B, H, W,
                c_void_p(ws_ptr), ws_bytes, max_in_flight, c_void_p(stream),
            )
        )

    def forward_view(self, x_ptr, x_strides, out_ptr, out_strides, qa_ptr, B, H, W, clamp, elem, window, ws_ptr, ws_bytes,
                     max_in_flight, stream) -> None:
        """mz_forward_view: `x_ptr` / `out_ptr` address element (0, 0, 0, 0) of each view (out: of the window), the strides count
        elements (image, channel, row, column; signed); `window` = (y0, x0, h, w) in output pixels or None; `elem` 1 = uint8."""
        xv, ov = view(x_ptr, x_strides), view(out_ptr, out_strides)
        win = _window_arg(window)
        check(
            lib().mz_forward_view(
                self._h, byref(xv), byref(ov), c_void_p(qa_ptr) if qa_ptr else None, B, H, W, int(clamp), int(elem), win,
                c_void_p(ws_ptr), ws_bytes, max_in_flight, c_void_p(stream),
            )
        )

    def flops_per_image(self, H: int, W: int) -> float:
        return float(lib().mz_flops_per_image(self._h, H, W))

    def schedule(self, B: int, H: int, W: int, want_qa: bool, cus: int = 256):
        """mz_debug_schedule (host only): the steps of one micro-batch of B images, in launch order, as a list of dicts with
        mz_debug_step's fields (off, bytes: tuples of in, second in, out; kernel: a str or None)."""
        n = lib().mz_debug_schedule(self._h, B, H, W, int(bool(want_qa)), cus, None, 0)  # how many
        if n < 0:
            check(n)
        steps = (MzDebugStep * n)()
        lib().mz_debug_schedule(self._h, B, H, W, int(bool(want_qa)), cus, steps, n)
        ints = [name for name, _ in MzDebugStep._fields_[:10]]
        return [dict({k: int(getattr(s, k)) for k in ints}, off=tuple(s.off), bytes=tuple(s.bytes),
                     kernel=s.kernel.decode() if s.kernel else None) for s in steps]

    def profile_enable(self, on: bool) -> None:
        check(lib().mz_profile_enable(self._h, int(on)))

    def profile_dump(self, path: str) -> None:
        check(lib().mz_profile_dump(self._h, str(path).encode()))

    def profile_read(self) -> dict:
        vals = [c_double() for _ in range(5)]
        check(lib().mz_profile_read(self._h, *[byref(v) for v in vals]))
        keys = ("conv_ms", "conv_flops", "conv_launches", "other_ms", "conv_bytes")
        return {k: v.value for k, v in zip(keys, vals)}
