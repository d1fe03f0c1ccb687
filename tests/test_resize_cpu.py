"""mz_resize without a GPU: the tap tables of mz_debug_resize_taps against the weight matrix torch itself uses, every refused argument
(refused before anything touches a device), the workspace size, and the Python layer's refusals and its torch backend.

The weight matrix of torch's antialiased resize of one axis is obtained by resizing the identity in float64: the height axis of
`interpolate(eye(n_in)[None, None], size=(n_in, n_out), antialias=True)` is the exact identity (its table is {0, 1, 0, 0}), so row r of
the result holds, for every output index i, the weight input sample r has in output i.  Both sides are float64 evaluations of one formula
with at most 66 taps: the gate is 1e-14 absolute (an independent restatement measured 1.6e-15), every row sums to 1 within 1e-15."""

import math
import re
from ctypes import byref, c_double, c_int, c_int32, c_int64, c_size_t, c_void_p
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from ultrazoom_amd import _ffi
from ultrazoom_amd.synth import synth_image

REPO = Path(__file__).resolve().parent.parent
MODES = {0: "bicubic", 1: "bilinear"}
AXES = [(64, 16), (37, 12), (48, 36), (33, 11), (24, 72), (41, 41), (64, 9), (64, 7), (17, 2), (19, 3), (160, 10), (8, 8)]
B, HIN, WIN, HOUT, WOUT = 2, 48, 64, 36, 48
FAKE = 0x10000  # never dereferenced: validation comes first


@pytest.mark.parametrize("filt", sorted(MODES))
@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_tap_tables_are_torchs_weight_matrix(axis, filt):
    n_in, n_out = axis
    eye = torch.eye(n_in, dtype=torch.float64)[None, None]
    matrix = F.interpolate(eye, size=(n_in, n_out), mode=MODES[filt], antialias=True, align_corners=False)[0, 0]  # [n_in, n_out]
    worst = 0.0
    for i in range(n_out):
        first, w = _ffi.resize_taps(n_in, n_out, filt, i)
        want = matrix[:, i]
        assert 1 <= len(w) <= _ffi.MZ_RESIZE_MAX_TAPS and 0 <= first and first + len(w) <= n_in
        got = torch.zeros(n_in, dtype=torch.float64)
        got[first:first + len(w)] = torch.tensor(w, dtype=torch.float64)
        worst = max(worst, float((got - want).abs().max()))
        assert abs(math.fsum(w) - 1.0) <= 1e-15, (i, math.fsum(w))
        # first and count, wherever torch's own row ends in nonzero weights (torch trims zero weights at the ends of its rows)
        nz = torch.nonzero(want).flatten()
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        assert first <= lo and hi <= first + len(w), (i, first, len(w), lo, hi)
        if w[0] != 0.0:
            assert first == lo, (i, first, lo)
        if w[-1] != 0.0:
            assert first + len(w) == hi, (i, first, len(w), hi)
        if n_in == n_out:
            assert sorted(abs(v) for v in w)[-1] == 1.0 and sum(1 for v in w if v != 0.0) == 1 and w[i - first] == 1.0, (i, w)
    print(f"{n_in} -> {n_out} {MODES[filt]}: worst weight difference {worst:.3e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("filt", sorted(MODES))
@pytest.mark.parametrize("shape", [((5, 1), (2, 1)), ((9, 7), (4, 1)), ((1, 7), (2, 3)), ((16, 16), (1, 1)), ((2, 2), (7, 9)), ((9, 7), (4, 3))],
                         ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_the_gpu_tests_checker_is_torchs_weight_matrices(shape, filt):
    """tests/resize_util.want64_of at the smallest shapes, outputs of one column included (which it runs transposed, around a fault
    of torch's kernel), against out = My^T x Mx with torch's own weight matrices (interpolate of an identity, as above)."""
    from resize_util import want64_of

    (hin, win), (hout, wout) = shape

    def matrix(n_in, n_out):  # [n_in, n_out]; n_out = 1: from the transposed identity as ONE ROW, so that no output of one column is asked for
        eye = torch.eye(n_in, dtype=torch.float64)[None, None]
        if n_out == 1:
            return F.interpolate(eye.transpose(-1, -2), size=(1, n_in), mode=MODES[filt], antialias=True, align_corners=False)[0, 0].transpose(0, 1)
        return F.interpolate(eye, size=(n_in, n_out), mode=MODES[filt], antialias=True, align_corners=False)[0, 0]

    x = torch.rand((3, 3, hin, win), generator=torch.Generator().manual_seed(hin * win), dtype=torch.float64)
    want = matrix(hin, hout).transpose(0, 1) @ x @ matrix(win, wout)
    assert float((want64_of(x, (hout, wout), MODES[filt]) - want).abs().max()) <= 1e-14


def test_the_formula_of_the_header_at_one_index():
    """64 -> 16 bicubic, i = 5: scale 4, support 8, center 22, first 14, count 16."""
    first, w = _ffi.resize_taps(64, 16, 0, 5)
    assert (first, len(w)) == (14, 16)

    def f(u):
        u = abs(u)
        return (1.5 * u - 2.5) * u * u + 1 if u < 1 else (((u - 5) * u + 8) * u - 4) * -0.5 if u < 2 else 0.0

    raw = [f((j + 14 - 22 + 0.5) / 4) for j in range(16)]
    for a, b in zip(w, raw):
        assert abs(a - b / sum(raw)) <= 1e-15


def view(data=FAKE, strides=None, h=HIN, w=WIN):
    return _ffi.MzImageView(c_void_p(data), (c_int64 * 4)(*(strides or (3 * h * w, h * w, w, 1))))


def call(x="dense", out="dense", elem=0, batch=B, hin=HIN, win=WIN, hout=HOUT, wout=WOUT, filt=0, window=None, ws=FAKE, ws_bytes=1 << 40):
    x = view() if x == "dense" else x
    out = view(h=hout, w=wout) if out == "dense" else out
    win_arr = (c_int32 * 4)(*window) if window is not None else None
    code = _ffi.lib().mz_resize(byref(x) if x is not None else None, byref(out) if out is not None else None, elem, batch, hin, win, hout,
                                wout, filt, 0, win_arr, c_void_p(ws) if ws else None, ws_bytes, None)
    return code, _ffi.lib().mz_last_error().decode()


def workspace(hin, win, hout, wout, filt):
    n = c_size_t()
    return _ffi.lib().mz_resize_workspace_bytes(hin, win, hout, wout, filt, byref(n)), int(n.value)


def out_view(strides):
    return _ffi.MzImageView(c_void_p(FAKE), (c_int64 * 4)(*strides))


DENSE_OUT = (3 * HOUT * WOUT, HOUT * WOUT, WOUT, 1)
REFUSED = {
    "null input view": dict(x=None),
    "null output view": dict(out=None),
    "null input data": dict(x=view(data=None)),
    "null output data": dict(out=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "filter -1": dict(filt=-1),
    "filter 2 (nearest is not offered)": dict(filt=2),
    "no images": dict(batch=0),
    "65536 images": dict(batch=65536),
    "no input rows": dict(hin=0),
    "no input columns": dict(win=0),
    "no output rows": dict(hout=0),
    "negative output width": dict(wout=-3),
    "rows shrink by 16.1": dict(hin=161, hout=10),
    "columns shrink by 17": dict(win=17 * 4, wout=4),
    "empty window": dict(window=(0, 0, 0, 5)),
    "window with a negative corner": dict(window=(-1, 0, 4, 4)),
    "window beyond the last row": dict(window=(HOUT - 3, 0, 4, 4)),
    "window beyond the last column": dict(window=(0, WOUT - 3, 4, 4)),
    "output channel stride 0": dict(out=out_view((DENSE_OUT[0], 0, WOUT, 1))),
    "output row stride 0": dict(out=out_view((DENSE_OUT[0], DENSE_OUT[1], 0, 1))),
    "output column stride 0": dict(out=out_view((DENSE_OUT[0], DENSE_OUT[1], WOUT, 0))),
    "output image stride 0 with two images": dict(out=out_view((0,) + DENSE_OUT[1:])),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_bad_arguments_are_refused_before_the_gpu(name):
    code, msg = call(**REFUSED[name])
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (name, code, msg)
    assert msg, name


def test_what_validation_lets_through_stops_at_the_workspace():
    """Still without a GPU call: the ratio-16 limit itself, enlarging without a bound, every element type and filter, a window, signed and
    zero input strides, an image stride of 0 for one image."""
    for args in (
        dict(hin=160, hout=10), dict(win=16 * 5, wout=5), dict(hin=2, win=2, hout=200, wout=300), dict(elem=1), dict(elem=2), dict(elem=3),
        dict(filt=1), dict(window=(HOUT - 4, WOUT - 4, 4, 4)), dict(window=(0, 0, HOUT, WOUT)), dict(batch=65535),
        dict(x=view(strides=(3 * HIN * WIN, -HIN * WIN, WIN, 1))), dict(x=view(strides=(0, 0, 0, 0))),
        dict(batch=1, out=out_view((0,) + DENSE_OUT[1:])),
    ):
        code, msg = call(ws_bytes=8, **args)
        assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL and "workspace too small" in msg, (args, code, msg)
    code, msg = call(ws=None)
    assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL, (code, msg)


def test_workspace_is_deterministic_and_holds_the_tables():
    for filt in (0, 1):
        for hin, win, hout, wout in [(HIN, WIN, HOUT, WOUT), (160, 40, 10, 40), (24, 40, 72, 120), (4320, 7680, 2160, 3840)]:
            code, n = workspace(hin, win, hout, wout, filt)
            assert code == 0 and (code, n) == workspace(hin, win, hout, wout, filt)
            taps_x = max(len(_ffi.resize_taps(win, wout, filt, i)[1]) for i in range(0, wout, max(1, wout // 50)))
            taps_y = max(len(_ffi.resize_taps(hin, hout, filt, i)[1]) for i in range(0, hout, max(1, hout // 50)))
            table = wout * (8 + 8 * taps_x) + hout * (8 + 8 * taps_y)  # {first, count} and float64 weights per output column / row
            assert table <= n <= 2 * table + 4096, (hin, win, hout, wout, n, table)
    for bad in ((0, 8, 8, 8, 0), (8, 8, 8, 0, 0), (161, 8, 10, 8, 0), (8, 8, 8, 8, 2)):
        assert workspace(*bad)[0] == _ffi.MZ_ERR_INVALID_ARGUMENT, bad
    assert _ffi.lib().mz_resize_workspace_bytes(8, 8, 8, 8, 0, None) == _ffi.MZ_ERR_INVALID_ARGUMENT


def test_debug_taps_refuses_bad_arguments():
    first, w = c_int(), (c_double * 66)()
    taps = _ffi.lib().mz_debug_resize_taps
    assert taps(160, 10, 0, 3, byref(first), w, 66) > 0
    for bad in ((161, 10, 0, 3, 66), (64, 16, 2, 3, 66), (64, 16, 0, 16, 66), (64, 16, 0, -1, 66), (0, 16, 0, 0, 66), (64, 16, 0, 3, 4)):
        assert taps(*bad[:4], byref(first), w, bad[4]) < 0, bad
        assert _ffi.lib().mz_last_error()
    assert taps(64, 16, 0, 3, None, w, 66) < 0 and taps(64, 16, 0, 3, byref(first), None, 66) < 0


def test_header_declares_the_entries_and_the_tile_constants():
    text = (REPO / "include" / "mewzoom_hip.h").read_text()
    assert re.search(r"\bint mz_resize_workspace_bytes\(int Hin, int Win, int Hout, int Wout, int filter, size_t\* bytes\);", text)
    assert re.search(r"\bint mz_resize\(const mz_image_view\* x, const mz_image_view\* out, int elem, int B, int Hin, int Win,", text)
    assert re.search(r"\bint mz_debug_resize_taps\(int n_in, int n_out, int filter, int i, int\* first, double\* w, int cap\);", text)
    assert re.search(r"#define MZ_RESIZE_BICUBIC 0\b", text) and re.search(r"#define MZ_RESIZE_BILINEAR 1\b", text)
    assert (_ffi.MZ_RESIZE_BICUBIC, _ffi.MZ_RESIZE_BILINEAR) == (0, 1)
    kernel = (REPO / "ultrazoom_amd" / "csrc" / "mz_resize.h").read_text()
    assert int(re.search(r"constexpr int kResizeTileH = (\d+);", kernel).group(1)) == 8
    assert int(re.search(r"constexpr int kResizeTileW = (\d+);", kernel).group(1)) == 32
    assert int(re.search(r"constexpr int kResizeMaxTaps = (\d+);", kernel).group(1)) == _ffi.MZ_RESIZE_MAX_TAPS


def test_resize_refusals_of_the_python_layer():
    from ultrazoom_amd.resize import resize

    x = synth_image(1, 24, 40, seed=1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        resize(x, (12, 20))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        resize(x[0], (12, 20))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        resize(x[:, :2], (12, 20))
    with pytest.raises(TypeError, match="unsupported dtype"):
        resize(x.double(), (12, 20))
    with pytest.raises(ValueError, match="filter"):
        resize(x, (12, 20), filter="nearest")


def test_upscale_to_refusals():
    from golden_util import GoldenCase
    from ultrazoom_amd import MewZoom

    case = GoldenCase("g3_4x_c16")
    m = MewZoom(**case.config).eval()
    x = case.image()
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.upscale_to(x, (72, 120))
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.upscale_to((x * 255).to(torch.uint8), (72, 120))
    with pytest.raises(RuntimeError, match=r"\(B, 3, H, W\)"):
        m.upscale_to(x[0], (72, 120))
    with pytest.raises(RuntimeError, match="should be the same"):
        m.upscale_to(x.double(), (72, 120))


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
def test_lr_from_hr_torch_backend_is_interpolate_of_the_cropped_image(filt):
    from ultrazoom_amd.evaluate import lr_from_hr

    hr = synth_image(2, 37, 45, seed=3)
    lr, cropped = lr_from_hr(hr, 4, filter=filt)
    assert cropped.shape == (2, 3, 36, 44) and cropped.data_ptr() == hr.data_ptr() and torch.equal(cropped, hr[:, :, :36, :44])
    assert lr.shape == (2, 3, 9, 11)
    assert torch.equal(lr, F.interpolate(hr[:, :, :36, :44], size=(9, 11), mode=filt, antialias=True, align_corners=False))
    with pytest.raises(ValueError, match="backend"):
        lr_from_hr(hr, 4, backend="numpy")
    with pytest.raises(ValueError, match="filter"):
        lr_from_hr(hr, 4, filter="nearest")
    with pytest.raises(RuntimeError, match="MI355X only"):
        lr_from_hr(hr, 4, backend="hip")


def test_evaluate_hr_is_evaluate_on_the_derived_pairs():
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr, lr_from_hr

    class Nearest:
        upscale_ratio = 2

        def upscale(self, x):
            return F.interpolate(x, scale_factor=2, mode="nearest")

    hrs = [synth_image(2, 49, 90, seed=5), synth_image(1, 48, 90, seed=6)]
    got = evaluate_hr(Nearest(), hrs)
    assert got == evaluate(Nearest(), [lr_from_hr(hr, 2) for hr in hrs])
    assert got["images"] == 3 and got["vif"] is not None and 10.0 < got["psnr"] < 60.0
