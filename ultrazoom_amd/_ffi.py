"""ctypes binding of libmewzoom_hip.so (include/mewzoom_hip.h).

There is deliberately no fallback: if the shared library is missing or a call fails, an exception
is raised.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or
``ultrazoom_amd/csrc/build.sh``).
"""

from __future__ import annotations

import ctypes
import os
import re
from contextlib import contextmanager
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_longlong, c_size_t, c_uint, c_uint8,
                    c_uint32, c_uint64, c_ulonglong, c_void_p)
from pathlib import Path

LIB_NAME = "libmewzoom_hip.so"
LIB_PATH = Path(__file__).resolve().parent / LIB_NAME

MZ_F32, MZ_BF16, MZ_F16 = 0, 1, 2

MZ_ERR_INVALID_ARGUMENT = -1
MZ_ERR_WORKSPACE_TOO_SMALL = -5

MZ_METRIC_SLOTS = 16  # doubles per image of mz_metrics' output (include/mewzoom_hip.h documents the slots)
MZ_METRIC_PSNR, MZ_METRIC_SSIM, MZ_METRIC_VIF = 1, 2, 4
MZ_METRIC_MIN_SIZE = {"ssim": 11, "vif": 41}  # pixels an image needs in both directions: the 11-tap window; four scales of 17, 9, 5, 3 taps
MZ_RESIZE_BICUBIC, MZ_RESIZE_BILINEAR = 0, 1
MZ_RESIZE_FILTERS = {"bicubic": MZ_RESIZE_BICUBIC, "bilinear": MZ_RESIZE_BILINEAR}
MZ_RESIZE_MAX_TAPS = 66  # taps of one output at the largest accepted ratio (n_in / n_out = 16, bicubic)
MZ_INTERP_NEAREST, MZ_INTERP_BILINEAR, MZ_INTERP_BICUBIC = 0, 1, 2
MZ_LUMA_STANDARDS = {"bt601": 0, "full": 1}  # studio range (MATLAB rgb2ycbcr, basicsr) / full range (JFIF, Pillow's "L")
MZ_YUV_MATRICES = {"bt601": 0, "bt709": 1}
MZ_YUV_RANGES = {"limited": 0, "full": 1}
MZ_YUV_SITINGS = {"left": 0, "center": 1}  # MPEG-2 / H.264 / HEVC; JPEG / MPEG-1
MZ_YCBCR_MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}  # the matrices of mz_ycbcr_to_rgb / mz_rgb_to_ycbcr
MZ_YCBCR_DEPTHS = (8, 10, 12, 16)
MZ_YCBCR_ALIGNS = {"low": 0, "high": 1}  # yuv420p10le and its kin; P010 / P012 / P016
MZ_YCBCR_SUBSAMPLINGS = {"420": 0, "422": 1, "444": 2}


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


# Every function of include/mewzoom_hip.h, in the header's own spelling and order (tests/test_ffi_cpu.py holds the two to each other).
PROTOTYPES = """
int mz_create(const mz_config* cfg, int dtype, mz_handle** out);
int mz_destroy(mz_handle* h);
int mz_num_weights(const mz_handle* h);
int mz_weight_info(const mz_handle* h, int index, const char** name, int64_t shape[4]);
int mz_set_weight(mz_handle* h, const char* name, const float* dev_f32, const int64_t* shape, int ndim, void* hip_stream);
int mz_weights_complete(const mz_handle* h);
int mz_workspace_bytes(const mz_handle* h, int B, int H, int W, int max_images_in_flight, size_t* bytes);
int mz_forward(mz_handle* h, const void* x, void* out_sr, float* out_qa, int B, int H, int W, int clamp, void* workspace,
    size_t workspace_bytes, int max_images_in_flight, void* hip_stream);
int mz_forward_u8(mz_handle* h, const uint8_t* x, uint8_t* out_sr, float* out_qa, int B, int H, int W, void* workspace,
    size_t workspace_bytes, int max_images_in_flight, void* hip_stream);
int mz_forward_view(mz_handle* h, const mz_image_view* x, const mz_image_view* out, float* out_qa, int B, int H, int W, int clamp,
    int elem, const int32_t window[4], void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream);
int mz_padded_channels(int c);
int mz_op_conv(int dtype, int kind, const void* in0, const void* in1, const float* w_dev_f32, float alpha, void* out, int B, int H, int W,
    int cin, int cout, int Hout, int Wout, int silu, void* hip_stream);
int mz_op_stem(int dtype, const void* x, const float* w_dev_f32, const float* b_dev_f32, void* out, int B, int H, int W, int cout,
    void* hip_stream);
int mz_op_final(int dtype, const void* feat, const void* img, const float* w_dev_f32, void* out, int B, int H, int W, int cin, int R,
    int clamp, void* hip_stream);
int mz_op_conv_mix(int dtype, const void* hid, const void* x, const float* w2_dev_f32, const float* wmix_dev_f32, float alpha, void* out,
    int B, int H, int W, int cin, int cout, void* hip_stream);
int mz_op_conv_film(int dtype, const void* in0, const float* w_dev_f32, const float* gamma_dev_f32, const float* beta_dev_f32, void* out,
    int B, int H, int W, int cin, int cout, int silu, void* hip_stream);
int mz_metrics_workspace_bytes(int B, int H, int W, int which, size_t* bytes);
int mz_metrics(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which, double data_range,
    double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream);
int mz_luma(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int standard, int clamp, void* hip_stream);
int mz_metrics_luma_workspace_bytes(int B, int H, int W, int which, size_t* bytes);
int mz_metrics_luma(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which, int standard,
    double data_range, double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream);
int mz_debug_luma_coeffs(int standard, double out[4]);
int mz_yuv420_to_rgb(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, const mz_image_view* out, int elem_out,
    int B, int H, int W, int matrix, int range, int siting, int clamp, void* hip_stream);
int mz_rgb_to_yuv420(const mz_image_view* x, int elem, const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr,
    int B, int H, int W, int matrix, int range, int siting, void* hip_stream);
int mz_debug_yuv_coeffs(int matrix, int range, double out[9]);
int mz_ycbcr_to_rgb(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, int depth, int align, int subsampling,
    const mz_image_view* out, int elem_out, int B, int H, int W, int matrix, int range, int siting, int clamp, void* hip_stream);
int mz_rgb_to_ycbcr(const mz_image_view* x, int elem, const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr,
    int depth, int align, int subsampling, int B, int H, int W, int matrix, int range, int siting, void* hip_stream);
int mz_debug_ycbcr_coeffs(int matrix, int range, int depth, double out[11]);
int mz_resize_workspace_bytes(int Hin, int Win, int Hout, int Wout, int filter, size_t* bytes);
int mz_resize(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win, int Hout, int Wout, int filter,
    int clamp, const int32_t window[4], void* workspace, size_t workspace_bytes, void* hip_stream);
int mz_debug_resize_taps(int n_in, int n_out, int filter, int i, int* first, double* w, int cap);
int mz_interpolate(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win, int Hout, int Wout, int mode,
    int clamp, const int32_t window[4], void* hip_stream);
int mz_debug_interp_taps(int n_in, int n_out, int mode, int i, int idx[4], double w[4]);
int mz_blur(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, void* hip_stream);
int mz_noise(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, uint64_t seed,
    uint64_t offset, void* hip_stream);
int mz_jpeg_workspace_bytes(int B, int H, int W, size_t* bytes);
int mz_jpeg(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int quality, void* workspace,
    size_t workspace_bytes, void* hip_stream);
int mz_debug_blur_weights(double sigma, double* w, int cap);
int mz_debug_jpeg_qtable(int quality, uint8_t* luma, uint8_t* chroma);
int mz_debug_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
int mz_dihedral_inverse(int k);
int mz_dihedral(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int k, void* hip_stream);
int mz_ensemble_workspace_bytes(int B, int H, int W, size_t* bytes);
int mz_ensemble_add(const mz_image_view* y, int elem, int B, int H, int W, int k, int first, void* workspace, size_t workspace_bytes,
    void* hip_stream);
int mz_ensemble_finish(const mz_image_view* out, int elem, int B, int H, int W, int n, int clamp, const int32_t window[4],
    void* workspace, size_t workspace_bytes, void* hip_stream);
int mz_alpha_fill_workspace_bytes(int B, int H, int W, size_t* bytes);
int mz_alpha_fill(const mz_image_view* rgb, const mz_image_view* alpha, const mz_image_view* out, int elem, int B, int H, int W,
    int premultiplied, void* workspace, size_t workspace_bytes, void* hip_stream);
int mz_alpha_merge(const mz_image_view* rgb, const mz_image_view* alpha, const mz_image_view* out_rgb, const mz_image_view* out_alpha,
    int elem, int B, int Hin, int Win, int Hout, int Wout, int mode, int premultiply, void* hip_stream);
int mz_debug_alpha_levels(int H, int W, int* hw, int cap);
int mz_feather_paste(const mz_image_view* src, const mz_image_view* dst, int elem, int B, int H, int W, int ramp_y, int ramp_x,
    void* hip_stream);
int mz_debug_feather_weight(int n, int k, double* w);
const char* mz_last_error(void);
const char* mz_version(void);
double mz_flops_per_image(const mz_handle* h, int H, int W);
int mz_profile_enable(mz_handle* h, int on);
int mz_profile_dump(mz_handle* h, const char* path);
int mz_profile_read(mz_handle* h, double* conv_ms, double* conv_flops, double* conv_launches, double* other_ms, double* conv_bytes);
int mz_debug_read(unsigned long long* host_dst);
const char* mz_debug_last_kernel(void);
int mz_debug_tile_list(int B, int tiles_y, int tiles_x, int ntiles, int gm, int gn, int blk4, int th, int tw, unsigned int* out, int cap);
const char* mz_debug_select(int dtype, int op, int cin, int cout, int B, int H, int W, int cus);
int mz_debug_schedule(const mz_handle* h, int B, int H, int W, int want_qa, int cus, mz_debug_step* out, int cap);
long long mz_debug_pack(int dtype, int op, int cin, int cout, int layout, long long* out, long long cap);
int mz_debug_store_hazard(int follower, int form, int wait_states, int dword, int iters, int blocks, unsigned int* counts_out);
"""

_SCALARS = {
    "int": c_int, "unsigned int": c_uint, "long long": c_longlong, "unsigned long long": c_ulonglong, "int32_t": c_int32,
    "int64_t": c_int64, "uint8_t": c_uint8, "uint32_t": c_uint32, "uint64_t": c_uint64, "size_t": c_size_t, "float": c_float,
    "double": c_double,
}
_POINTERS = {
    "char*": c_char_p, "char**": POINTER(c_char_p), "mz_handle*": c_void_p, "mz_handle**": POINTER(c_void_p),
    "mz_config*": POINTER(MzConfig), "mz_image_view*": POINTER(MzImageView), "mz_debug_step*": POINTER(MzDebugStep),
    "size_t*": POINTER(c_size_t),  # the result of every *_workspace_bytes entry: always byref(c_size_t()) or None
}


def _ctype(spelling: str):
    """The ctypes type of a C type as the header spells it (`T name[N]` arrives as `T*`).  Any other pointer to a scalar or to void than
    those of _POINTERS is c_void_p: a device address as an int, a ctypes array, byref(...) and None all pass.  A spelling not listed here
    is an error, never a default."""
    key = re.sub(r"\bconst ", "", spelling)
    if key in _SCALARS:
        return _SCALARS[key]
    if key in _POINTERS:
        return _POINTERS[key]
    if key.endswith("*") and (key[:-1] in _SCALARS or key[:-1] == "void"):
        return c_void_p
    raise TypeError(f"no ctypes type is stated for the C type {spelling!r}")


def _parse(prototypes: str) -> dict:
    """{name: (restype, argtypes)} of C prototypes, one `;` after each."""
    table = {}
    for text in prototypes.split(";")[:-1]:
        result, name, params = re.fullmatch(r"(.+?)\s*\b(mz_\w+)\((.*)\)", " ".join(text.split())).groups()
        argtypes = []
        for param in ([] if params == "void" else params.split(", ")):
            spelling, _, array = re.fullmatch(r"(.+?[ *])(\w+)(\[\d+\])?", param).groups()
            argtypes.append(_ctype(spelling.strip() + ("*" if array else "")))
        table[name] = (_ctype(result), argtypes)
    return table


SIGNATURES = _parse(PROTOTYPES)


def _declare(lib) -> None:
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # a function the library does not export is an error here
        fn.restype, fn.argtypes = restype, argtypes


_lib = None


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


def pair(t):
    """(address of element (0, 0, 0, 0), element strides) of a tensor: the two arguments that name a view in the functions below."""
    return t.data_ptr(), t.stride()


@contextmanager
def image_frame(x, out=None, want=None, need=None):
    """The frame of a tensor-level image entry around its call of the library: inside, x's device is the current one, and the frame hands
    over (out, (workspace address, workspace bytes) or (), the current stream as an int).  `out` is held to the shape `want` by
    check_same_batch before anything touches the device; without one it is a new dense tensor of that shape and of x's dtype (want =
    None: the entry has no image output).  `need`, a function that returns a number of bytes, asks for a uint8 workspace of that size."""
    import torch

    if out is not None:
        check_same_batch(x, out, want)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ws = ()
        if need is not None:
            nbytes = need()
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)  # lives until the call inside the frame is enqueued
            ws = (scratch.data_ptr(), nbytes)
        if out is None and want is not None:
            out = torch.empty(want, dtype=x.dtype, device=x.device)
        yield out, ws, stream


def view(ptr, strides) -> MzImageView:
    """An mz_image_view: the address of element (0, 0, 0, 0) and the element strides (image, channel, row, column; signed)."""
    return MzImageView(c_void_p(ptr), (c_int64 * 4)(*[int(v) for v in strides]))


def _window_arg(window):
    """`window` = (y0, x0, h, w) or None as the `const int32_t window[4]` of an entry."""
    return (c_int32 * 4)(*[int(v) for v in window]) if window is not None else None


def make_config(cfg: dict) -> MzConfig:
    return MzConfig(**{k: int(cfg[k]) for k, _ in MzConfig._fields_})


def _call(entry: str, *args) -> None:
    """One call of a status-returning entry.  A view or a config is passed as it is (ctypes takes its address for a POINTER parameter), a
    device address or a stream as an int; a status other than 0 raises."""
    check(getattr(lib(), entry)(*args))


def _bytes(entry: str, *args) -> int:
    """What a *_workspace_bytes entry writes to its `size_t* bytes`."""
    out = c_size_t()
    _call(entry, *args, byref(out))
    return int(out.value)


def _count(n: int) -> int:
    """The count a host-only mz_debug_* entry returns; negative: its status."""
    if n < 0:
        check(n)
    return n


def metrics_workspace_bytes(B: int, H: int, W: int, which: int) -> int:
    return _bytes("mz_metrics_workspace_bytes", B, H, W, which)


def metrics(pred_ptr, pred_strides, target_ptr, target_strides, elem, B, H, W, which, data_range, sigma_n_sq, out_ptr, ws_ptr, ws_bytes,
            stream) -> None:
    """mz_metrics: the two views as for Handle.forward_view; `elem` 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8."""
    _call("mz_metrics", view(pred_ptr, pred_strides), view(target_ptr, target_strides), int(elem), B, H, W, int(which), float(data_range),
          float(sigma_n_sq), out_ptr, ws_ptr, ws_bytes, stream)


def luma_standard(standard) -> int:
    """The `standard` code of the luma entries: "bt601" -> 0, "full" -> 1."""
    if standard not in MZ_LUMA_STANDARDS:
        raise ValueError(f"luma standard is 'bt601' (studio range) or 'full' (full range), got {standard!r}")
    return MZ_LUMA_STANDARDS[standard]


def resize_filter(filter_) -> int:
    """The `filter` code of mz_resize: "bicubic" -> 0, "bilinear" -> 1."""
    if filter_ not in tuple(MZ_RESIZE_FILTERS):
        raise ValueError(f"filter is 'bicubic' or 'bilinear', got {filter_!r}")
    return MZ_RESIZE_FILTERS[filter_]


def luma(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, standard, clamp, stream) -> None:
    """mz_luma: x a view of [B,3,H,W], out a view of [B,1,H,W], as for `resize`; `standard` 0 bt601, 1 full; no workspace."""
    _call("mz_luma", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, H, W, int(standard), bool(clamp), stream)


def luma_coeffs(standard: int):
    """mz_debug_luma_coeffs (host only): [off, kr, kg, kb], the constants the kernels compile."""
    out = (c_double * 4)()
    _call("mz_debug_luma_coeffs", int(standard), out)
    return [float(v) for v in out]


def yuv_codes(matrix, range_, siting):
    """The (matrix, range, siting) codes of the YCbCr entries, from their names."""
    for what, value, table in (("matrix", matrix, MZ_YUV_MATRICES), ("range", range_, MZ_YUV_RANGES), ("siting", siting, MZ_YUV_SITINGS)):
        if value not in tuple(table):
            raise ValueError(f"{what} is {' or '.join(repr(k) for k in table)}, got {value!r}")
    return MZ_YUV_MATRICES[matrix], MZ_YUV_RANGES[range_], MZ_YUV_SITINGS[siting]


def yuv420_to_rgb(y, cb, cr, out, elem_out, B, H, W, matrix, range_, siting, clamp, stream) -> None:
    """mz_yuv420_to_rgb: y, cb, cr and out are (address, strides) pairs of the uint8 planes [B,1,H,W], [B,1,Hc,Wc] twice and of the
    [B,3,H,W] result of element type `elem_out`; no workspace."""
    _call("mz_yuv420_to_rgb", view(*y), view(*cb), view(*cr), view(*out), int(elem_out), B, H, W, int(matrix), int(range_), int(siting),
          bool(clamp), stream)


def rgb_to_yuv420(x, elem, y, cb, cr, B, H, W, matrix, range_, siting, stream) -> None:
    """mz_rgb_to_yuv420: x the (address, strides) pair of a [B,3,H,W] view of element type `elem`; y, cb, cr those of the planes written."""
    _call("mz_rgb_to_yuv420", view(*x), int(elem), view(*y), view(*cb), view(*cr), B, H, W, int(matrix), int(range_), int(siting), stream)


def yuv_coeffs(matrix: int, range_: int):
    """mz_debug_yuv_coeffs (host only): [Yoff, 1/Sy, 1/Sc, a_r, a_b, g_r, g_b, Sy, Sc], the constants the kernels compile."""
    out = (c_double * 9)()
    _call("mz_debug_yuv_coeffs", int(matrix), int(range_), out)
    return [float(v) for v in out]


def ycbcr_codes(depth, align, subsampling, matrix, range_, siting):
    """((depth, align, subsampling), (matrix, range, siting)) codes of the mz_ycbcr entries, from their names."""
    if depth not in MZ_YCBCR_DEPTHS:
        raise ValueError(f"depth is 8, 10, 12 or 16, got {depth!r}")
    for what, value, table in (("align", align, MZ_YCBCR_ALIGNS), ("subsampling", subsampling, MZ_YCBCR_SUBSAMPLINGS),
                               ("matrix", matrix, MZ_YCBCR_MATRICES), ("range", range_, MZ_YUV_RANGES), ("siting", siting, MZ_YUV_SITINGS)):
        if value not in tuple(table):
            raise ValueError(f"{what} is {' or '.join(repr(k) for k in table)}, got {value!r}")
    return ((int(depth), MZ_YCBCR_ALIGNS[align], MZ_YCBCR_SUBSAMPLINGS[subsampling]),
            (MZ_YCBCR_MATRICES[matrix], MZ_YUV_RANGES[range_], MZ_YUV_SITINGS[siting]))


def ycbcr_to_rgb(y, cb, cr, depth, align, subsampling, out, elem_out, B, H, W, matrix, range_, siting, clamp, stream) -> None:
    """mz_ycbcr_to_rgb: y, cb, cr and out are (address, strides) pairs of the uint8 (depth 8) or uint16 planes and of the [B,3,H,W] result of
    element type `elem_out`; no workspace."""
    _call("mz_ycbcr_to_rgb", view(*y), view(*cb), view(*cr), int(depth), int(align), int(subsampling), view(*out), int(elem_out), B, H, W,
          int(matrix), int(range_), int(siting), bool(clamp), stream)


def rgb_to_ycbcr(x, elem, y, cb, cr, depth, align, subsampling, B, H, W, matrix, range_, siting, stream) -> None:
    """mz_rgb_to_ycbcr: x the (address, strides) pair of a [B,3,H,W] view of element type `elem`; y, cb, cr those of the planes written."""
    _call("mz_rgb_to_ycbcr", view(*x), int(elem), view(*y), view(*cb), view(*cr), int(depth), int(align), int(subsampling), B, H, W,
          int(matrix), int(range_), int(siting), stream)


def ycbcr_coeffs(matrix: int, range_: int, depth: int):
    """mz_debug_ycbcr_coeffs (host only): the nine values of yuv_coeffs at `depth`, then the chroma midpoint and the largest code."""
    out = (c_double * 11)()
    _call("mz_debug_ycbcr_coeffs", int(matrix), int(range_), int(depth), out)
    return [float(v) for v in out]


def metrics_luma_workspace_bytes(B: int, H: int, W: int, which: int) -> int:
    return _bytes("mz_metrics_luma_workspace_bytes", B, H, W, which)


def metrics_luma(pred_ptr, pred_strides, target_ptr, target_strides, elem, B, H, W, which, standard, data_range, sigma_n_sq, out_ptr, ws_ptr,
                 ws_bytes, stream) -> None:
    """mz_metrics_luma: `metrics` on the float64 Y planes of the two [B,3,H,W] views."""
    _call("mz_metrics_luma", view(pred_ptr, pred_strides), view(target_ptr, target_strides), int(elem), B, H, W, int(which), int(standard),
          float(data_range), float(sigma_n_sq), out_ptr, ws_ptr, ws_bytes, stream)


def resize_workspace_bytes(Hin: int, Win: int, Hout: int, Wout: int, filter_: int) -> int:
    return _bytes("mz_resize_workspace_bytes", Hin, Win, Hout, Wout, int(filter_))


def resize(x_ptr, x_strides, out_ptr, out_strides, elem, B, Hin, Win, Hout, Wout, filter_, clamp, window, ws_ptr, ws_bytes, stream) -> None:
    """mz_resize: the two views as for Handle.forward_view (out: of the window); `elem` 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8;
    `window` = (y0, x0, h, w) in pixels of the Hout x Wout result, or None."""
    _call("mz_resize", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, Hin, Win, Hout, Wout, int(filter_), bool(clamp),
          _window_arg(window), ws_ptr, ws_bytes, stream)


def resize_taps(n_in: int, n_out: int, filter_: int, i: int):
    """mz_debug_resize_taps (host only): (first, [w_0 .. w_{count-1}]) of output index i of one axis."""
    first = c_int()
    w = (c_double * MZ_RESIZE_MAX_TAPS)()
    count = _count(lib().mz_debug_resize_taps(n_in, n_out, int(filter_), i, byref(first), w, MZ_RESIZE_MAX_TAPS))
    return int(first.value), [float(w[j]) for j in range(count)]


def interpolate(x_ptr, x_strides, out_ptr, out_strides, elem, B, Hin, Win, Hout, Wout, mode, clamp, window, stream) -> None:
    """mz_interpolate: the two views and the window as for `resize`; `mode` 0 nearest, 1 bilinear, 2 bicubic (A = -0.75); no workspace."""
    _call("mz_interpolate", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, Hin, Win, Hout, Wout, int(mode), bool(clamp),
          _window_arg(window), stream)


def interp_taps(n_in: int, n_out: int, mode: int, i: int):
    """mz_debug_interp_taps (host only): ([idx_0 ..], [w_0 ..]) of output index i of one axis, 1, 2 or 4 taps."""
    idx, w = (c_int * 4)(), (c_double * 4)()
    count = _count(lib().mz_debug_interp_taps(n_in, n_out, int(mode), i, idx, w))
    return [int(idx[j]) for j in range(count)], [float(w[j]) for j in range(count)]


def blur(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, sigma, stream) -> None:
    """mz_blur: the two views as for `resize`; `elem` 0..2 = MZ_F32 / MZ_BF16 / MZ_F16, 3 = uint8."""
    _call("mz_blur", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, H, W, float(sigma), stream)


def noise(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, sigma, seed, offset, stream) -> None:
    """mz_noise: `seed` and `offset` are taken modulo 2^64; out may be the same view as x."""
    _call("mz_noise", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, H, W, float(sigma), int(seed) & (2**64 - 1),
          int(offset) & (2**64 - 1), stream)


def jpeg_workspace_bytes(B: int, H: int, W: int) -> int:
    return _bytes("mz_jpeg_workspace_bytes", B, H, W)


def jpeg(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, quality, ws_ptr, ws_bytes, stream) -> None:
    """mz_jpeg: the round trip at `quality` 1..100 on a workspace of `jpeg_workspace_bytes(B, H, W)` bytes."""
    _call("mz_jpeg", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, H, W, int(quality), ws_ptr, ws_bytes, stream)


def blur_weights(sigma: float):
    """mz_debug_blur_weights (host only): the k = 2 * int(3 sigma) + 1 normalised weights the kernel is handed."""
    w = (c_double * 31)()
    k = _count(lib().mz_debug_blur_weights(float(sigma), w, 31))
    return [float(w[j]) for j in range(k)]


def jpeg_qtable(quality: int):
    """mz_debug_jpeg_qtable (host only): (luminance, chrominance), 64 integers each, row-major."""
    a, b = (c_uint8 * 64)(), (c_uint8 * 64)()
    _call("mz_debug_jpeg_qtable", int(quality), a, b)
    return list(a), list(b)


def philox(counter, key):
    """mz_debug_philox (host only): the four words of one Philox4x32-10 block, from the function the noise kernel compiles."""
    out = (c_uint32 * 4)()
    _call("mz_debug_philox", (c_uint32 * 4)(*counter), (c_uint32 * 2)(*key), out)
    return [int(v) for v in out]


def dihedral_inverse(k: int) -> int:
    """mz_dihedral_inverse (host only): the orientation that undoes orientation k; negative outside 0..7."""
    return int(lib().mz_dihedral_inverse(int(k)))


def dihedral(x_ptr, x_strides, out_ptr, out_strides, elem, B, H, W, k, stream) -> None:
    """mz_dihedral: out, a view of [B,3,H',W'], receives T(x, k) of the [B,3,H,W] view x; the views as for `resize`."""
    _call("mz_dihedral", view(x_ptr, x_strides), view(out_ptr, out_strides), int(elem), B, H, W, int(k), stream)


def ensemble_workspace_bytes(B: int, H: int, W: int) -> int:
    return _bytes("mz_ensemble_workspace_bytes", B, H, W)


def ensemble_add(y_ptr, y_strides, elem, B, H, W, k, first, ws_ptr, ws_bytes, stream) -> None:
    """mz_ensemble_add: the pass result y, a view in ITS orientation ([B,3,W,H] when k & 4), turned back and stored in (`first`) or added
    to the float32 accumulator of the [B,3,H,W] result."""
    _call("mz_ensemble_add", view(y_ptr, y_strides), int(elem), B, H, W, int(k), bool(first), ws_ptr, ws_bytes, stream)


def ensemble_finish(out_ptr, out_strides, elem, B, H, W, n, clamp, window, ws_ptr, ws_bytes, stream) -> None:
    """mz_ensemble_finish: the mean of the n results added, into out (a view of the window, as for `resize`)."""
    _call("mz_ensemble_finish", view(out_ptr, out_strides), int(elem), B, H, W, int(n), bool(clamp), _window_arg(window), ws_ptr, ws_bytes,
          stream)


def alpha_fill_workspace_bytes(B: int, H: int, W: int) -> int:
    return _bytes("mz_alpha_fill_workspace_bytes", B, H, W)


def alpha_fill(rgb, alpha, out, elem, B, H, W, premultiplied, ws_ptr, ws_bytes, stream) -> None:
    """mz_alpha_fill: rgb, alpha and out are (address, strides) pairs of the [B,3,H,W] colour, the [B,1,H,W] alpha plane and the [B,3,H,W]
    result, all of element type `elem`; the workspace holds `alpha_fill_workspace_bytes(B, H, W)` bytes."""
    _call("mz_alpha_fill", view(*rgb), view(*alpha), view(*out), int(elem), B, H, W, bool(premultiplied), ws_ptr, ws_bytes, stream)


def alpha_merge(rgb, alpha, out_rgb, out_alpha, elem, B, Hin, Win, Hout, Wout, mode, premultiply, stream) -> None:
    """mz_alpha_merge: alpha [B,1,Hin,Win] and out_alpha [B,1,Hout,Wout] as (address, strides) pairs; rgb and out_rgb ([B,3,Hout,Wout]) are
    pairs with `premultiply` and may be None without it; `mode` as for `interpolate`; no workspace."""
    _call("mz_alpha_merge", view(*rgb) if rgb is not None else None, view(*alpha), view(*out_rgb) if out_rgb is not None else None,
          view(*out_alpha), int(elem), B, Hin, Win, Hout, Wout, int(mode), bool(premultiply), stream)


def alpha_levels(H: int, W: int):
    """mz_debug_alpha_levels (host only): [(H_l, W_l)] of the pyramid of an H x W image, level 0 first, down to (1, 1)."""
    n = _count(lib().mz_debug_alpha_levels(H, W, None, 0))
    hw = (c_int * (2 * n))()
    _count(lib().mz_debug_alpha_levels(H, W, hw, n))
    return [(int(hw[2 * l]), int(hw[2 * l + 1])) for l in range(n)]


def feather_paste(src, dst, elem, B, H, W, ramp_y, ramp_x, stream) -> None:
    """mz_feather_paste: src and dst are (address, strides) pairs of two [B,3,H,W] views of element type `elem`; the ramps count
    positions from the top and the left edge; no workspace."""
    _call("mz_feather_paste", view(*src), view(*dst), int(elem), B, H, W, int(ramp_y), int(ramp_x), stream)


def feather_weight(n: int, k: int) -> float:
    """mz_debug_feather_weight (host only): omega(n, k), from the functions the kernel compiles."""
    w = c_double()
    _call("mz_debug_feather_weight", int(n), int(k), byref(w))
    return float(w.value)


class Handle:
    """Owns one mz_handle."""

    def __init__(self, cfg: dict, dtype_code_: int):
        self._h = c_void_p()
        _call("mz_create", make_config(cfg), dtype_code_, byref(self._h))
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
        out = []
        for i in range(lib().mz_num_weights(self._h)):
            name = c_char_p()
            shape = (c_int64 * 4)()
            ndim = _count(lib().mz_weight_info(self._h, i, byref(name), shape))
            out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim))))
        return out

    def set_weight(self, name: str, dev_ptr: int, shape, stream: int) -> None:
        arr = (c_int64 * 4)(*list(shape) + [0] * (4 - len(shape)))
        _call("mz_set_weight", self._h, name.encode(), dev_ptr, arr, len(shape), stream)

    def weights_complete(self) -> None:
        _call("mz_weights_complete", self._h)

    def workspace_bytes(self, B: int, H: int, W: int, max_in_flight: int = 0) -> int:
        return _bytes("mz_workspace_bytes", self._h, B, H, W, max_in_flight)

    def forward(self, x_ptr, sr_ptr, qa_ptr, B, H, W, clamp, ws_ptr, ws_bytes, max_in_flight, stream) -> None:
        _call("mz_forward", self._h, x_ptr, sr_ptr, qa_ptr or None, B, H, W, int(clamp), ws_ptr, ws_bytes, max_in_flight, stream)

    def forward_u8(self, x_ptr, sr_ptr, qa_ptr, B, H, W, ws_ptr, ws_bytes, max_in_flight, stream) -> None:
        _call("mz_forward_u8", self._h, x_ptr, sr_ptr, qa_ptr or None, B, H, W, ws_ptr, ws_bytes, max_in_flight, stream)

    def forward_view(self, x_ptr, x_strides, out_ptr, out_strides, qa_ptr, B, H, W, clamp, elem, window, ws_ptr, ws_bytes,
                     max_in_flight, stream) -> None:
        """mz_forward_view: `x_ptr` / `out_ptr` address element (0, 0, 0, 0) of each view (out: of the window), the strides count
        elements (image, channel, row, column; signed); `window` = (y0, x0, h, w) in output pixels or None; `elem` 1 = uint8."""
        _call("mz_forward_view", self._h, view(x_ptr, x_strides), view(out_ptr, out_strides), qa_ptr or None, B, H, W, int(clamp), int(elem),
              _window_arg(window), ws_ptr, ws_bytes, max_in_flight, stream)

    def flops_per_image(self, H: int, W: int) -> float:
        return float(lib().mz_flops_per_image(self._h, H, W))

    def schedule(self, B: int, H: int, W: int, want_qa: bool, cus: int = 256):
        """mz_debug_schedule (host only): the steps of one micro-batch of B images, in launch order, as a list of dicts with
        mz_debug_step's fields (off, bytes: tuples of in, second in, out; kernel: a str or None)."""
        n = _count(lib().mz_debug_schedule(self._h, B, H, W, bool(want_qa), cus, None, 0))  # how many
        steps = (MzDebugStep * n)()
        lib().mz_debug_schedule(self._h, B, H, W, bool(want_qa), cus, steps, n)
        ints = [name for name, _ in MzDebugStep._fields_[:10]]
        return [dict({k: int(getattr(s, k)) for k in ints}, off=tuple(s.off), bytes=tuple(s.bytes),
                     kernel=s.kernel.decode() if s.kernel else None) for s in steps]

    def profile_enable(self, on: bool) -> None:
        _call("mz_profile_enable", self._h, int(on))

    def profile_dump(self, path: str) -> None:
        _call("mz_profile_dump", self._h, str(path).encode())

    def profile_read(self) -> dict:
        vals = [c_double() for _ in range(5)]
        _call("mz_profile_read", self._h, *[byref(v) for v in vals])
        keys = ("conv_ms", "conv_flops", "conv_launches", "other_ms", "conv_bytes")
        return {k: v.value for k, v in zip(keys, vals)}

