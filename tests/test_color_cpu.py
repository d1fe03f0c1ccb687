"""The luma entries without a GPU: the constants mz_debug_luma_coeffs returns against tests/color_ref.py, the reference itself against exact
rational arithmetic, the declarations, the workspace sizes, every refused argument of mz_luma and mz_metrics_luma (refused before anything
touches a device), the Python layer's refusals, and the torch backend of evaluate(..., luma=, shave=) against a computation by hand."""

import math
import re
import struct
from ctypes import byref, c_double, c_int, c_size_t, c_void_p
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import color_ref
from ultrazoom_amd import _ffi
from ultrazoom_amd.evaluate import PSNR, SSIM, VIF, evaluate, evaluate_hr, luma_plane
from ultrazoom_amd.metrics import MetricsAccumulator, image_metrics
from ultrazoom_amd.synth import synth_image

REPO = Path(__file__).resolve().parent.parent
B, H, W = 2, 48, 64
DENSE3, DENSE1 = (3 * H * W, H * W, W, 1), (H * W, H * W, W, 1)
FAKE, FAKE2 = 0x10000, 0x40000000  # never dereferenced: validation comes first; far enough apart for any shape used here
INVALID, TOO_SMALL = _ffi.MZ_ERR_INVALID_ARGUMENT, _ffi.MZ_ERR_WORKSPACE_TOO_SMALL


def bits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


# ---- the constants and the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("standard", ["bt601", "full"])
def test_the_library_compiles_the_constants_python_divides(standard):
    got = _ffi.luma_coeffs(color_ref.CODE[standard])
    assert [bits(v) for v in got] == [bits(v) for v in color_ref.COEFFS[standard]], (got, color_ref.COEFFS[standard])
    from ultrazoom_amd.evaluate import LUMA_COEFFS

    assert [bits(v) for v in LUMA_COEFFS[standard]] == [bits(v) for v in got]


def test_bad_standard_and_null_argument_of_the_debug_entry():
    lib = _ffi.lib()
    out = (c_double * 4)()
    assert lib.mz_debug_luma_coeffs(2, out) == INVALID and "standard" in lib.mz_last_error().decode()
    assert lib.mz_debug_luma_coeffs(-1, out) == INVALID
    assert lib.mz_debug_luma_coeffs(0, None) == INVALID


def exact_byte(standard: str, r: int, g: int, b: int) -> int:
    """the byte of the EXACT Y: floor(Y * 255 + 1/2) in rational arithmetic (Y of a uint8 colour is inside [0, 1])"""
    if standard == "bt601":
        y255 = 16 + Fraction(65481 * r + 128553 * g + 24966 * b, 255000)
    else:
        y255 = Fraction(299 * r + 587 * g + 114 * b, 1000)
    return math.floor(y255 + Fraction(1, 2))


def test_white_and_black_in_studio_range():
    x = torch.tensor([[255, 0], [255, 0], [255, 0]], dtype=torch.uint8).reshape(1, 3, 1, 2)
    assert color_ref.luma_expected(x, "bt601", "u8", 0).flatten().tolist() == [235, 16]
    y = color_ref.luma_f64(x, "bt601").flatten()
    assert abs(y[0] - 235 / 255) <= 2 ** -52 and y[1] == 16.0 / 255.0


def test_greys_and_primaries_against_exact_rational_arithmetic():
    """The 256 greys and the three primaries: no exact Y * 255 of these is within 1 / 255000 of k + 1/2 (asserted), so the float64
    arithmetic must give the byte of the exact value."""
    colours = [(g, g, g) for g in range(256)] + [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    x = torch.tensor(colours, dtype=torch.uint8).T.reshape(1, 3, 1, -1).contiguous()
    for standard in ("bt601", "full"):
        ties = {tuple(int(v) for v in c) for c in color_ref.u8_ties(standard)}
        assert not ties & set(colours)
        want = [exact_byte(standard, *c) for c in colours]
        assert color_ref.luma_expected(x, standard, "u8", 0).flatten().tolist() == want
        assert color_ref.luma_expected(x, standard, "u8", 1).flatten().tolist() == want  # uint8 clamps whatever it is told
    assert [exact_byte("bt601", *c) for c in colours[256:]] == [81, 145, 41]  # the studio-range primaries of the standard
    assert color_ref.luma_expected(x[..., :256], "full", "u8", 0).flatten().tolist() == list(range(256))  # "full" of a grey g is g


def test_the_search_for_uint8_ties_finds_what_the_reference_says():
    for standard in ("bt601", "full"):
        assert color_ref.tie_census(standard) == color_ref.TIE_CENSUS[standard]
        c = color_ref.u8_ties(standard)[::97]
        assert all(exact_byte(standard, *(int(v) for v in px)) - 1 <= int(got) <= exact_byte(standard, *(int(v) for v in px))
                   for px, got in zip(c, color_ref.luma_expected(torch.from_numpy(c.T.reshape(1, 3, 1, -1).copy()), standard, "u8", 0).flatten()))


def test_the_store_rule_of_each_type():
    y = np.array([[-0.25, 0.0, 2.0 ** -30, 0.5 + 2.0 ** -12, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.5, 65519.99, 65520.0, math.inf, -math.inf, math.nan]])
    f16 = color_ref.store(y, "f16", 0).flatten().tolist()
    assert f16[3] == 0.5 and f16[6] == 65504.0 and f16[7] == math.inf and math.isnan(f16[10])  # a tie to even; the overflow tie
    assert color_ref.store(y, "bf16", 0).flatten().tolist()[4] == 1.0 + 2.0 ** -7  # ONE rounding: via float32 it would be a tie, to 1.0
    assert color_ref.store(y, "f32", 1).flatten().tolist() == [0.0, 0.0, 2.0 ** -30, 0.5 + 2.0 ** -12, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert color_ref.store(y, "u8", 0).flatten().tolist() == [0, 0, 0, 128, 255, 255, 255, 255, 255, 0, 0]


def test_the_planted_inputs_are_in_the_images():
    x = color_ref.image(1, 5, 64, "f16")
    assert bool(x.isnan().any()) and bool(x.isinf().any()) and float(x[~x.isnan() & ~x.isinf()].max()) == 65504.0
    assert bool(((x != 0) & (x.abs() < 2.0 ** -14)).any()) and bool((x < 0).any()) and bool((x[~x.isnan()] > 1).any())
    assert bool(torch.signbit(x[0, :, 0, 0]).all()) and bool((x[0, :, 0, 0] == 0).all())  # the -0 pixel
    ties = {tuple(int(v) for v in c) for s in ("bt601", "full") for c in color_ref.u8_ties(s)}
    u = color_ref.image(1, 5, 64, "u8")[0].reshape(3, -1).T.tolist()
    assert sum(tuple(px) in ties for px in u[:29]) >= 24
    # no finite float16 input overflows: the largest Y there is
    huge = torch.full((1, 3, 1, 1), 65504.0, dtype=torch.float16)
    assert color_ref.luma_expected(huge, "full", "f16", 0).item() == 65504.0 and color_ref.luma_expected(huge, "bt601", "f16", 0).item() < 65504.0


# ---- declarations ------------------------------------------------------------------------------------------------------------------------
CTYPE = {"int": c_int, "double": c_double, "size_t": c_size_t}


def test_the_header_prototypes_match_the_ctypes_declarations():
    text = (REPO / "include" / "mewzoom_hip.h").read_text()
    lib = _ffi.lib()
    for name in ("mz_luma", "mz_metrics_luma_workspace_bytes", "mz_metrics_luma", "mz_debug_luma_coeffs"):
        m = re.search(rf"\bint {name}\(([^;]*)\);", text)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        fn = getattr(lib, name)
        assert fn.restype is c_int and len(fn.argtypes) == len(params), (name, params)
        for p, t in zip(params, fn.argtypes):
            if "*" in p or "[" in p:
                assert t is c_void_p or hasattr(t, "contents"), (name, p, t)  # a pointer of some kind
                if "mz_image_view" in p:
                    assert t._type_ is _ffi.MzImageView
                elif "double" in p and t is not c_void_p:
                    assert t._type_ is c_double
                elif "size_t" in p:
                    assert t._type_ is c_size_t
            else:
                assert t is CTYPE[p.split()[0]], (name, p, t)
    assert [n for n in ("mz_luma", "mz_metrics_luma") if n not in text.split("THE VIEW REFUSALS")[1].split("typedef")[0]] == []


def test_units_list_names_the_new_translation_unit():
    assert "mz_color" in (REPO / "ultrazoom_amd" / "csrc" / "units.sh").read_text()
    import ultrazoom_amd

    assert ultrazoom_amd.rgb_to_y is __import__("ultrazoom_amd.color", fromlist=["rgb_to_y"]).rgb_to_y and "rgb_to_y" in ultrazoom_amd.__all__


# ---- refusals of the C entries -------------------------------------------------------------------------------------------------------------
def luma(x="dense", out="dense", elem=0, batch=B, h=H, w=W, standard=0):
    x = _ffi.view(FAKE, DENSE3) if x == "dense" else x
    out = _ffi.view(FAKE2, DENSE1) if out == "dense" else out
    lib = _ffi.lib()
    code = lib.mz_luma(byref(x) if x is not None else None, byref(out) if out is not None else None, elem, batch, h, w, standard, 0, None)
    return code, lib.mz_last_error().decode()


LUMA_REFUSED = {
    "null input view": (dict(x=None), "null"),
    "null output view": (dict(out=None), "null"),
    "null input data": (dict(x=_ffi.view(None, DENSE3)), "null data"),
    "null output data": (dict(out=_ffi.view(None, DENSE1)), "null data"),
    "elem -1": (dict(elem=-1), "elem"),
    "elem 4": (dict(elem=4), "elem"),
    "standard -1": (dict(standard=-1), "standard"),
    "standard 2": (dict(standard=2), "standard"),
    "no images": (dict(batch=0), "B"),
    "65536 images": (dict(batch=65536), "B"),
    "no rows": (dict(h=0), "H, W"),
    "2^28 + 1 columns": (dict(w=(1 << 28) + 1), "2^28"),
    "output row stride 0": (dict(out=_ffi.view(FAKE2, (H * W, 1, 0, 1))), "row stride is 0"),
    "output column stride 0": (dict(out=_ffi.view(FAKE2, (H * W, 1, W, 0))), "column stride is 0"),
    "output image stride 0 with two images": (dict(out=_ffi.view(FAKE2, (0, 1, W, 1))), "image stride is 0"),
    "out is x's green plane": (dict(out=_ffi.view(FAKE + 4 * H * W, DENSE1)), "overlap"),
    "out is x's first plane": (dict(out=_ffi.view(FAKE, DENSE1)), "overlap"),
    "out ends inside x": (dict(out=_ffi.view(FAKE - 4 * (B * H * W) + 4, DENSE1)), "overlap"),
    "x reversed over out": (dict(x=_ffi.view(FAKE2 + 4 * (B * H * W + 3 * B * H * W - 2), (-3 * H * W, -H * W, -W, -1))), "overlap"),
    "a byte range beyond 63 bits": (dict(x=_ffi.view(FAKE, (1 << 62, H * W, W, 1))), "63 bits"),
}


@pytest.mark.parametrize("name", sorted(LUMA_REFUSED))
def test_mz_luma_refuses(name):
    kw, word = LUMA_REFUSED[name]
    code, msg = luma(**kw)
    assert code == INVALID and word in msg, (name, code, msg)


def metrics_luma(pred="dense", target="dense", elem=0, batch=B, h=H, w=W, which=7, standard=0, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
    pred = _ffi.view(FAKE, DENSE3) if pred == "dense" else pred
    target = _ffi.view(FAKE2, DENSE3) if target == "dense" else target
    lib = _ffi.lib()
    code = lib.mz_metrics_luma(byref(pred) if pred is not None else None, byref(target) if target is not None else None, elem, batch, h, w,
                               which, standard, -1.0, 2.0, c_void_p(out) if out else None, c_void_p(ws) if ws else None, ws_bytes, None)
    return code, lib.mz_last_error().decode()


def luma_workspace(batch, h, w, which):
    n = c_size_t()
    code = _ffi.lib().mz_metrics_luma_workspace_bytes(batch, h, w, which, byref(n))
    return code, int(n.value)


METRICS_REFUSED = {
    "null pred view": (dict(pred=None), INVALID, "null"),
    "null target view": (dict(target=None), INVALID, "null"),
    "null pred data": (dict(pred=_ffi.view(None, DENSE3)), INVALID, "null data"),
    "elem -1": (dict(elem=-1), INVALID, "elem"),
    "elem 4": (dict(elem=4), INVALID, "elem"),
    "standard 2": (dict(standard=2), INVALID, "standard"),
    "standard -1": (dict(standard=-1), INVALID, "standard"),
    "which 0": (dict(which=0), INVALID, "which"),
    "which 8": (dict(which=8), INVALID, "which"),
    "no images": (dict(batch=0), INVALID, "B, H, W"),
    "65536 images": (dict(batch=65536), INVALID, "65535"),
    "10 rows with SSIM": (dict(h=10, which=2), INVALID, "11 x 11"),
    "40 columns with VIF": (dict(w=40, which=4), INVALID, "41 x 41"),
    "planes beyond 2^62 bytes": (dict(batch=65535, h=1 << 28, w=1 << 28, which=1), INVALID, "2^62"),
    "null out": (dict(out=None), INVALID, "out_dev"),
    "null workspace": (dict(ws=None), TOO_SMALL, "workspace"),
    "workspace one byte short": (dict(ws_bytes=color_ref.metrics_plan_bytes(B, H, W, 7, 1, True) - 1), TOO_SMALL, "workspace"),
    "the workspace of one RGB-less plane": (dict(ws_bytes=color_ref.metrics_plan_bytes(B, H, W, 7, 1, False)), TOO_SMALL, "workspace"),
}


@pytest.mark.parametrize("name", sorted(METRICS_REFUSED))
def test_mz_metrics_luma_refuses(name):
    kw, want, word = METRICS_REFUSED[name]
    code, msg = metrics_luma(**kw)
    assert code == want and word in msg, (name, code, msg)


def test_workspace_query_refuses_what_the_call_refuses():
    assert _ffi.lib().mz_metrics_luma_workspace_bytes(B, H, W, 7, None) == INVALID
    for args in [(0, H, W, 7), (B, 10, W, 2), (B, H, 40, 4), (B, H, W, 0), (65535, 1 << 28, 1 << 28, 1)]:
        assert luma_workspace(*args)[0] == INVALID, args
    assert luma_workspace(1, 1 << 28, 1 << 28, 1) == (0, color_ref.metrics_plan_bytes(1, 1 << 28, 1 << 28, 1, 1, True))  # 2^60 bytes of planes


SHAPES = [(1, 1, 1), (2, 11, 11), (1, 26, 42), (3, 27, 43), (1, 41, 41), (3, 75, 93), (2, 49, 51), (16, 4320, 7680), (1, 170, 512), (5, 171, 9)]


def test_luma_workspace_is_the_plan_of_one_plane_and_the_two_planes():
    for Bn, h, w in SHAPES:
        for which in (1, 2, 4, 3, 7):
            if (which & 2 and min(h, w) < 11) or (which & 4 and min(h, w) < 41):
                continue
            assert luma_workspace(Bn, h, w, which) == (0, color_ref.metrics_plan_bytes(Bn, h, w, which, 1, True)), (Bn, h, w, which)
            one = color_ref.metrics_plan_bytes(Bn, h, w, which, 1, False)
            assert luma_workspace(Bn, h, w, which)[1] - one == (16 * Bn * h * w + 255) // 256 * 256


# mz_metrics_workspace_bytes(B, H, W, which) as the parent commit returned it
RGB_WORKSPACE = {
    (1, 1, 1, 1): 512, (2, 11, 11, 3): 3328, (1, 26, 42, 3): 3840, (3, 27, 43, 3): 10496, (1, 41, 41, 7): 23808, (3, 75, 93, 7): 294912,
    (2, 49, 51, 7): 68096, (2, 49, 51, 4): 67584, (16, 4320, 7680, 1): 327936, (16, 4320, 7680, 7): 8420788224, (1, 170, 512, 2): 24576,
    (5, 171, 9, 1): 102656, (1, 1080, 1920, 7): 32549120,
}


def test_rgb_workspace_is_what_it_was():
    for (Bn, h, w, which), want in RGB_WORKSPACE.items():
        assert _ffi.metrics_workspace_bytes(Bn, h, w, which) == want == color_ref.metrics_plan_bytes(Bn, h, w, which), (Bn, h, w, which)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    from ultrazoom_amd.color import rgb_to_y

    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="luma standard"):
        image_metrics(x, x, luma="bt709")
    with pytest.raises(ValueError, match="luma standard"):
        rgb_to_y(x, "ycbcr")
    with pytest.raises(ValueError, match="luma standard"):
        MetricsAccumulator(luma="y")
    with pytest.raises(ValueError, match="11 x 11"):
        image_metrics(x, x, which=("psnr", "ssim"), luma="bt601", shave=27)  # 10 x 10 are left
    with pytest.raises(ValueError, match="41 x 41"):
        image_metrics(x, x, shave=12)  # 40 x 40 are left
    with pytest.raises(ValueError, match="leaves nothing"):
        image_metrics(x, x, which=("psnr",), shave=32)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="shave"):
            image_metrics(x, x, shave=bad)
    with pytest.raises(RuntimeError, match="MI355X only"):  # what the shave leaves is fine: the call goes on to the device check
        image_metrics(x, x, luma="bt601", shave=11)
    with pytest.raises(RuntimeError, match="MI355X only"):
        rgb_to_y(x)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        rgb_to_y(torch.zeros(1, 1, 8, 8))
    for fn in (evaluate, evaluate_hr):
        with pytest.raises(ValueError, match="luma"):
            fn(None, [], luma="bt709")
    with pytest.raises(ValueError, match="luma standard"):
        luma_plane(x, "bt709")


def test_luma_plane_is_the_reference_plane_to_three_roundings():
    for dt in ("f32", "bf16", "f16", "u8"):
        x = color_ref.image(2, 7, 129, dt, special=False)
        for standard in ("bt601", "full"):
            got, want = luma_plane(x, standard), torch.from_numpy(color_ref.luma_f64(x, standard))
            assert got.dtype == torch.float64 and got.shape == (2, 1, 7, 129)
            # |Y| < 2 and every product < 1: the fused sum has three roundings of at most 2^-53, the plain one those and three of 2^-54
            assert float((got - want).abs().max()) <= 15 * 2.0 ** -54


class Nearest:
    upscale_ratio = 2

    def upscale(self, x):
        return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")


@pytest.mark.parametrize("luma, shave", [("bt601", 2), ("full", 0), (None, 3), ("bt601", 4)])
def test_evaluate_torch_backend_matches_a_computation_by_hand(luma, shave):
    hr = synth_image(3, 52, 48, seed=5)
    noisy = (hr + 0.2 * (synth_image(3, 52, 48, seed=6, smooth=False) - 0.5)).clamp(0, 1)
    lr = noisy[:, :, ::2, ::2]
    pairs = [(lr[:2], hr[:2]), (lr[2:], hr[2:])]
    got = evaluate(Nearest(), pairs, luma=luma, shave=shave, baseline=True)
    # by hand: crop, the plane of color_ref, the meters
    meters = {"": (PSNR(1.0), SSIM(), VIF()), "bicubic_": (PSNR(1.0), SSIM(), VIF())}
    for x, y in pairs:
        for key, img in (("", Nearest().upscale(x)), ("bicubic_", torch.nn.functional.interpolate(x.double(), size=y.shape[-2:], mode="bicubic",
                                                                                                  align_corners=False).clamp(0, 1).float())):
            def cut(t):
                t = t[..., shave:t.shape[-2] - shave, shave:t.shape[-1] - shave]
                return t if luma is None else torch.from_numpy(color_ref.luma_f64(t.contiguous(), luma))

            p, t = cut(img), cut(y)
            assert p.shape[1] == (3 if luma is None else 1) and p.shape[-2:] == (52 - 2 * shave, 48 - 2 * shave)
            for m in meters[key][: 3 if min(p.shape[-2:]) >= 41 else 2]:
                m.update(p, t)
    assert got["images"] == 3
    for key, (psnr, ssim, vif) in meters.items():
        assert math.isclose(got[key + "psnr"], psnr.compute(), rel_tol=1e-12), (key, got, psnr.compute())
        assert math.isclose(got[key + "ssim"], ssim.compute(), rel_tol=1e-9), (key, got, ssim.compute())
        if 48 - 2 * shave >= 41:
            assert math.isclose(got[key + "vif"], vif.compute(), rel_tol=1e-9), (key, got, vif.compute())
        else:
            assert got[key + "vif"] is None
    assert set(got) == {"psnr", "ssim", "vif", "images", "bicubic_psnr", "bicubic_ssim", "bicubic_vif"}
    if luma is None and shave == 0:
        return
    plain = evaluate(Nearest(), pairs, baseline=True)
    assert plain["psnr"] != got["psnr"] and plain == evaluate(Nearest(), pairs, baseline=True, luma=None, shave=0)


def test_evaluate_hr_passes_luma_and_shave_on():
    hr = synth_image(2, 52, 48, seed=9)
    got = evaluate_hr(Nearest(), [hr], luma="bt601", shave=2)
    from ultrazoom_amd.evaluate import lr_from_hr

    assert got == evaluate(Nearest(), [lr_from_hr(hr, 2)], luma="bt601", shave=2) != evaluate(Nearest(), [lr_from_hr(hr, 2)])
