"""mz_interpolate without a GPU: the taps of mz_debug_interp_taps against the weight matrix torch itself uses (an identity pushed through
its float64 CPU kernels), every refused argument of the C entry (refused before anything touches the GPU: the pointers here are fake),
the header against the ctypes declarations, the Python layer's argument errors, and the bicubic baseline of evaluate() against a by-hand
computation."""

import math
import re
from ctypes import byref, c_double, c_int, c_int32, c_int64, c_void_p
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from interp_util import MODE, MODES, nearest_index
from ultrazoom_amd import _ffi
from ultrazoom_amd.synth import synth_image

REPO = Path(__file__).resolve().parent.parent
FAKE, FAKE2 = 0x10000, 1 << 44  # never dereferenced: validation comes first; far enough apart for the largest shapes used here
B, HIN, WIN, HOUT, WOUT = 2, 24, 40, 72, 120


# ---- the taps --------------------------------------------------------------------------------------------------------------------------
def weight_matrix(n_in: int, n_out: int, mode: int) -> torch.Tensor:
    m = [[0.0] * n_in for _ in range(n_out)]
    for i in range(n_out):
        idx, w = _ffi.interp_taps(n_in, n_out, mode, i)
        assert len(idx) == len(w) == (1, 2, 4)[mode] and all(0 <= j < n_in for j in idx), (n_in, n_out, mode, i, idx)
        for j, v in zip(idx, w):
            m[i][j] += v  # (taps clamped to one edge pixel add up, as torch's do)
    return torch.tensor(m, dtype=torch.float64)


@pytest.mark.parametrize("mode", MODES)
def test_taps_are_torchs_weight_matrix(mode):
    """For all n_in, n_out in 1..64: the matrix built from the taps equals F.interpolate of a float64 identity (the columns of the identity
    are images of one row; the output's rows are the matrix's columns).  Nearest exactly; the others to 1e-12 (measured: 5e-15)."""
    worst = 0.0
    for n_in in range(1, 65):
        eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, 1, n_in)  # [1, C = source index, 1, W = n_in]
        for n_out in range(1, 65):
            kw = {} if mode == "nearest" else {"align_corners": False}
            want = F.interpolate(eye, size=(1, n_out), mode=mode, **kw)[0, :, 0, :].t()  # [n_out, n_in]
            got = weight_matrix(n_in, n_out, MODE[mode])
            if mode == "nearest":
                assert torch.equal(got, want), (n_in, n_out)
            else:
                worst = max(worst, float((got - want).abs().max()))
    print(f"{mode}: largest difference to torch's float64 weights {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("n_in, n_out", [(1920, 1080), (1080, 1920), (4097, 77), (77, 4097), (6000, 5999), (5999, 6000)])
def test_nearest_indices_are_torchs_float32_rule(n_in, n_out):
    want = nearest_index(n_in, n_out).tolist()
    got = [_ffi.interp_taps(n_in, n_out, 0, i)[0][0] for i in range(n_out)]
    assert got == want


@pytest.mark.parametrize("n", [1, 2, 3, 41, 64, 4097, 1 << 28])
def test_equal_sizes_have_exact_tables(n):
    for i in sorted({0, 1 % n, n // 2, n - 1}):
        assert _ffi.interp_taps(n, n, 0, i) == ([i], [1.0])
        idx, w = _ffi.interp_taps(n, n, 1, i)
        assert idx == [i, min(i + 1, n - 1)] and w == [1.0, 0.0]
        idx, w = _ffi.interp_taps(n, n, 2, i)
        assert idx == [min(max(i - 1 + k, 0), n - 1) for k in range(4)] and w == [0.0, 1.0, 0.0, 0.0]


def test_bicubic_weights_by_hand():
    """w = {c2(t + 1), c1(t), c1(1 - t), c2(2 - t)} with A = -0.75 sums to one and has negative outer weights; 4 -> 8 samples, output 3:
    src = 1.25, t = 1 / 4, taps 0..3, the weights worked out by hand (dyadic: exact)"""
    for i in range(8):
        idx, w = _ffi.interp_taps(5, 40, 2, i + 8)
        assert abs(sum(w) - 1.0) <= 1e-15 and w[0] <= 0.0 and w[3] <= 0.0
    assert _ffi.interp_taps(4, 8, 2, 3) == ([0, 1, 2, 3], [-0.10546875, 0.87890625, 0.26171875, -0.03515625])
    assert _ffi.interp_taps(4, 8, 2, 0) == ([0, 0, 0, 1], [-0.03515625, 0.26171875, 0.87890625, -0.10546875])  # src = -0.25, t = 3 / 4


def test_debug_taps_refuses_bad_arguments():
    idx, w = (c_int * 4)(), (c_double * 4)()
    taps = _ffi.lib().mz_debug_interp_taps
    assert taps(24, 72, 2, 3, idx, w) == 4 and taps(24, 72, 1, 3, idx, w) == 2 and taps(24, 72, 0, 3, idx, w) == 1
    for bad in ((24, 72, 3, 3), (24, 72, -1, 3), (0, 72, 2, 0), (24, 0, 2, 0), (24, 72, 2, 72), (24, 72, 2, -1), ((1 << 28) + 1, 72, 2, 0)):
        assert taps(*bad, idx, w) == _ffi.MZ_ERR_INVALID_ARGUMENT, bad
        assert _ffi.lib().mz_last_error()
    assert taps(24, 72, 2, 3, None, w) < 0 and taps(24, 72, 2, 3, idx, None) < 0


# ---- the C entry's refusals ------------------------------------------------------------------------------------------------------------
def dense(h, w):
    return (3 * h * w, h * w, w, 1)


def view(data=FAKE, strides=None, h=HIN, w=WIN):
    return _ffi.MzImageView(c_void_p(data), (c_int64 * 4)(*(strides or dense(h, w))))


def call(x="dense", out="dense", elem=0, batch=B, hin=HIN, win=WIN, hout=HOUT, wout=WOUT, mode=2, clamp=0, window=None):
    x = view() if x == "dense" else x
    out = view(data=FAKE2, h=hout, w=wout) if out == "dense" else out
    win_arr = (c_int32 * 4)(*window) if window is not None else None
    code = _ffi.lib().mz_interpolate(byref(x) if x is not None else None, byref(out) if out is not None else None, elem, batch, hin, win, hout,
                                     wout, mode, clamp, win_arr, None)
    return code, _ffi.lib().mz_last_error().decode()


DO = dense(HOUT, WOUT)
X_BYTES = 4 * B * 3 * HIN * WIN
REFUSED = {
    "null input view": dict(x=None),
    "null output view": dict(out=None),
    "null input data": dict(x=view(data=None)),
    "null output data": dict(out=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "mode -1": dict(mode=-1),
    "mode 3": dict(mode=3),
    "no images": dict(batch=0),
    "65536 images": dict(batch=65536),
    "no input rows": dict(hin=0),
    "no input columns": dict(win=0),
    "no output rows": dict(hout=0),
    "negative output width": dict(wout=-3),
    "input rows beyond 2^28": dict(hin=(1 << 28) + 1),
    "input columns beyond 2^28": dict(win=(1 << 28) + 1),
    "output rows beyond 2^28": dict(hout=(1 << 28) + 1),
    "output columns beyond 2^28": dict(wout=(1 << 28) + 1),
    "empty window": dict(window=(0, 0, 0, 5)),
    "window with a negative corner": dict(window=(-1, 0, 4, 4)),
    "window beyond the last row": dict(window=(HOUT - 3, 0, 4, 4)),
    "window beyond the last column": dict(window=(0, WOUT - 3, 4, 4)),
    "output channel stride 0": dict(out=view(FAKE2, (DO[0], 0, WOUT, 1))),
    "output row stride 0": dict(out=view(FAKE2, (DO[0], DO[1], 0, 1))),
    "output column stride 0": dict(out=view(FAKE2, (DO[0], DO[1], WOUT, 0))),
    "output image stride 0 with two images": dict(out=view(FAKE2, (0,) + DO[1:])),
    "in place": dict(out=view(FAKE, DO)),
    "out begins inside x": dict(out=view(FAKE + X_BYTES - 4, DO)),
    "out ends inside x": dict(out=view(FAKE - 4 * B * 3 * HOUT * WOUT + 4, DO)),
    "a window of out ends inside x": dict(out=view(FAKE - 4 * (DO[0] + 2 * DO[1] + 3 * WOUT + 3), DO), window=(5, 6, 4, 4)),
    "x inside a strided out": dict(out=view(FAKE - 64, tuple(2 * s for s in DO))),
    "a byte range beyond 63 bits": dict(x=view(strides=((1 << 62), HIN * WIN, WIN, 1))),
    "clamp with nearest": dict(mode=0, clamp=1),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_bad_arguments_are_refused_before_the_gpu(name):
    code, msg = call(**REFUSED[name])
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (name, code, msg)
    assert msg, name
    if name != "clamp with nearest":
        assert not msg.startswith("clamp"), (name, msg)


def test_what_validation_lets_through_reaches_the_last_check():
    """Still without a GPU call.  The entry has no workspace to be short of, so these calls carry the one thing its LAST check refuses --
    a clamp with nearest: arguments every earlier check accepts come back with that message.  Any sizes up and down without a ratio
    limit, every element type, windows, signed and zero input strides, an image stride of 0 for one image, ranges that touch."""
    for args in (
        dict(), dict(hin=1 << 28, win=1, hout=1, wout=1 << 28), dict(hin=1000, hout=3), dict(hin=2, win=2, hout=200, wout=300), dict(elem=1),
        dict(elem=2), dict(elem=3), dict(window=(HOUT - 4, WOUT - 4, 4, 4)), dict(window=(0, 0, HOUT, WOUT)), dict(batch=65535),
        dict(x=view(strides=(3 * HIN * WIN, -HIN * WIN, WIN, 1))), dict(x=view(strides=(0, 0, 0, 0))),
        dict(x=view(data=FAKE + 4 * (3 * HIN * WIN - 1), strides=(3 * HIN * WIN, -HIN * WIN, -WIN, -1)), batch=1),
        dict(batch=1, out=view(FAKE2, (0,) + DO[1:])), dict(out=view(FAKE + X_BYTES, DO)),
        dict(out=view(FAKE - 4 * (DO[0] + 2 * DO[1] + 3 * WOUT + 3) - 4, DO), window=(5, 6, 4, 4)),
    ):
        code, msg = call(mode=0, clamp=1, **args)
        assert code == _ffi.MZ_ERR_INVALID_ARGUMENT and msg.startswith("clamp with mode 0"), (args, code, msg)


def test_header_declares_the_entries_and_the_tile_constants():
    text = (REPO / "include" / "mewzoom_hip.h").read_text()
    assert re.search(r"\bint mz_interpolate\(const mz_image_view\* x, const mz_image_view\* out, int elem, int B, int Hin, int Win,\s+"
                     r"int Hout, int Wout, int mode, int clamp, const int32_t window\[4\], void\* hip_stream\);", text)
    assert re.search(r"\bint mz_debug_interp_taps\(int n_in, int n_out, int mode, int i, int idx\[4\], double w\[4\]\);", text)
    for name, value in (("NEAREST", 0), ("BILINEAR", 1), ("BICUBIC", 2)):
        assert re.search(rf"#define MZ_INTERP_{name}\s+{value}\b", text) and getattr(_ffi, f"MZ_INTERP_{name}") == value
    lib = _ffi.lib()
    assert len(lib.mz_interpolate.argtypes) == 12 and lib.mz_interpolate.restype is c_int
    assert len(lib.mz_debug_interp_taps.argtypes) == 6 and lib.mz_debug_interp_taps.restype is c_int
    assert text.index("int mz_debug_resize_taps(") < text.index("int mz_interpolate(") < text.index("int mz_blur(")  # after the resampling section
    units = (REPO / "ultrazoom_amd" / "csrc" / "units.sh").read_text()
    assert re.search(r"kernel_units=\([^)]*\bmz_interp\b", units)
    kernel = (REPO / "ultrazoom_amd" / "csrc" / "mz_interp.h").read_text()
    th, tw, rows = (int(re.search(rf"constexpr int kInterp{n} = (\d+);", kernel).group(1)) for n in ("TileH", "TileW", "StageRows"))
    assert tw % 16 == 0 and tw & (tw - 1) == 0       # a tile row is whole 16-byte chunks of every element type
    assert rows >= th // 2 + 3                       # the separable path serves every ratio from 2 upwards
    assert 4 * 12 * (th + tw) + 8 * rows * (tw + 16) <= 32 * 1024  # the LDS of the bicubic instantiations: five workgroups a CU


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_python_layer():
    import ultrazoom_amd
    from ultrazoom_amd.interpolate import interpolate

    assert ultrazoom_amd.interpolate is interpolate
    x = synth_image(1, 24, 40, seed=1)
    with pytest.raises(RuntimeError, match="MI355X only.*no CPU path"):
        interpolate(x, (48, 80))
    with pytest.raises(RuntimeError, match="MI355X only"):
        interpolate((x * 255).to(torch.uint8), scale_factor=2, mode="nearest")
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        interpolate(x[0], (48, 80))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        interpolate(x[:, :2], (48, 80))
    with pytest.raises(TypeError, match="unsupported dtype"):
        interpolate(x.double(), (48, 80))
    with pytest.raises(ValueError, match="mode"):
        interpolate(x, (48, 80), mode="area")
    with pytest.raises(ValueError, match="no clamp"):
        interpolate(x, (48, 80), mode="nearest", clamp=True)
    with pytest.raises(ValueError, match="exactly one"):
        interpolate(x)
    with pytest.raises(ValueError, match="exactly one"):
        interpolate(x, (48, 80), 2)
    for bad in (1.5, 2.0, 0, -2, True, "2"):
        with pytest.raises(ValueError, match="positive integer"):
            interpolate(x, scale_factor=bad)
    assert "torch.nn.functional" not in (REPO / "ultrazoom_amd" / "interpolate.py").read_text()


def test_upscale_and_bicubic_has_no_cpu_path():
    from golden_util import GoldenCase
    from ultrazoom_amd import MewZoom

    case = GoldenCase("g3_4x_c16")
    m = MewZoom(**case.config).eval()
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.upscale_and_bicubic(case.image())
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.upscale_and_bicubic((case.image() * 255).to(torch.uint8))


# ---- evaluate(..., baseline=True) ----------------------------------------------------------------------------------------------------------
class Doubler:
    """stands in for a model on the CPU: pixel replication by two"""

    upscale_ratio = 2

    def upscale(self, x):
        return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def pairs():
    blocks = (torch.rand((1, 3, 12, 16), generator=torch.Generator().manual_seed(3)) > 0.5).float()
    hr = [synth_image(2, 48, 64, seed=5), blocks.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)]  # the second: 0 / 1 edges
    return [(F.avg_pool2d(y, 2), y) for y in hr]


def test_the_torch_baseline_is_the_by_hand_computation():
    from ultrazoom_amd.evaluate import evaluate, ssim_per_image, vif_per_image

    got = evaluate(Doubler(), pairs(), baseline=True)
    base = [F.interpolate(x.double(), size=y.shape[-2:], mode="bicubic", align_corners=False).clamp(0, 1).float() for x, y in pairs()]
    assert float(F.interpolate(pairs()[1][0], scale_factor=2, mode="bicubic").min()) < -0.05  # (the clamp has something to do)
    sq = sum(float(((b.double() - y.double()) ** 2).sum()) for b, (_, y) in zip(base, pairs()))
    n = sum(y.numel() for _, y in pairs())
    assert got["bicubic_psnr"] == pytest.approx(10.0 * math.log10(n / sq), rel=1e-12)
    assert got["bicubic_ssim"] == pytest.approx(float(torch.cat([ssim_per_image(b, y) for b, (_, y) in zip(base, pairs())]).mean()), rel=1e-12)
    assert got["bicubic_vif"] == pytest.approx(float(torch.cat([vif_per_image(b, y) for b, (_, y) in zip(base, pairs())]).mean()), rel=1e-12)
    assert got["images"] == 3 and got["bicubic_psnr"] != got["psnr"]  # (the baseline is not the model's own result again)


def test_the_torch_baseline_of_uint8_and_16_bit_images():
    from ultrazoom_amd.evaluate import bicubic_baseline

    x = synth_image(1, 12, 20, seed=2)
    want = F.interpolate(x.double(), size=(24, 40), mode="bicubic", align_corners=False).clamp(0, 1)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        xd = x.to(dt)
        got = bicubic_baseline(xd, (24, 40))
        assert got.dtype == dt and got.shape == (1, 3, 24, 40)
        assert torch.equal(got, F.interpolate(xd.double(), size=(24, 40), mode="bicubic", align_corners=False).clamp(0, 1).to(dt))
    x8 = (x * 255).round().to(torch.uint8)
    got = bicubic_baseline(x8, (24, 40))
    assert got.dtype == torch.uint8 and int((got.double() - want * 255).abs().max()) <= 1
    assert torch.equal(got, torch.floor(F.interpolate(x8.double() / 255, size=(24, 40), mode="bicubic", align_corners=False).clamp(0, 1) * 255 + 0.5).to(torch.uint8))


def test_without_baseline_the_results_are_todays():
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr

    plain = evaluate(Doubler(), pairs())
    assert list(plain) == ["psnr", "ssim", "vif", "images"] and plain == evaluate(Doubler(), pairs(), "torch", 1, False)
    with_base = evaluate(Doubler(), pairs(), baseline=True)
    assert {k: v for k, v in with_base.items() if not k.startswith("bicubic_")} == plain
    assert sorted(k for k in with_base if k.startswith("bicubic_")) == ["bicubic_psnr", "bicubic_ssim", "bicubic_vif"]
    hr = [y for _, y in pairs()]
    plain_hr = evaluate_hr(Doubler(), hr)
    assert list(plain_hr) == ["psnr", "ssim", "vif", "images"]
    assert {k: v for k, v in evaluate_hr(Doubler(), hr, baseline=True).items() if not k.startswith("bicubic_")} == plain_hr
    small = [(torch.rand(1, 3, 10, 12), torch.rand(1, 3, 20, 24))]  # below 41 pixels: no VIF on either side
    assert evaluate(Doubler(), small, baseline=True)["bicubic_vif"] is None
    with pytest.raises(ValueError, match="device only"):
        evaluate_hr(Doubler(), hr, degrade=object(), baseline=True)
    text = (REPO / "ultrazoom_amd" / "evaluate.py").read_text()
    assert "def upscale" not in text and "def forward" not in text
