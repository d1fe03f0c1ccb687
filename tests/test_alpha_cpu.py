"""The alpha entries without a GPU: the pyramid and the workspace of the library against the restatement (tests/alpha_ref.py), every
refusal of mz_alpha_fill and mz_alpha_merge -- returned before anything touches the GPU, on views at addresses that are never
dereferenced -- the properties of the restatement itself, and the bicubic weights that keep an opaque image opaque."""

import math
import re
from ctypes import byref, c_int, c_size_t
from pathlib import Path

import numpy as np
import pytest
import torch

import alpha_ref
import color_ref
import image_exact
from ultrazoom_amd import _ffi

INVALID, TOO_SMALL = _ffi.MZ_ERR_INVALID_ARGUMENT, _ffi.MZ_ERR_WORKSPACE_TOO_SMALL
REPO = Path(__file__).resolve().parent.parent
FAKE, FAKE2, FAKE3, WS = 0x10000, 0x40000000, 0x50000000, 0x70000000  # never dereferenced: validation comes first
B, H, W, R = 2, 6, 10, 2
PYRAMID_SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (9, 8), (17, 33), (1080, 1920), (1 << 28, 1 << 28), (1 << 28, 1), (3, 1 << 28)]


# ---- the pyramid -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", PYRAMID_SIZES, ids=lambda v: str(v))
def test_levels_and_workspace_are_those_of_the_restatement(h, w):
    want = alpha_ref.levels(h, w)
    assert _ffi.alpha_levels(h, w) == want and want[0] == (h, w) and want[-1] == (1, 1)
    assert len(want) == 1 + max(math.ceil(math.log2(h)), math.ceil(math.log2(w)))
    for batch in (1, 3):
        assert _ffi.alpha_fill_workspace_bytes(batch, h, w) == alpha_ref.workspace_bytes(batch, h, w)
    # a cap shorter than the pyramid: the count all the same, the first levels only
    hw = (c_int * 4)(-1, -1, -1, -1)
    assert _ffi.lib().mz_debug_alpha_levels(h, w, hw, 1) == len(want) and tuple(hw) == (h, w, -1, -1)


def test_the_pyramid_entries_refuse_bad_arguments():
    lib = _ffi.lib()
    out = c_size_t()
    for args in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 28) + 1, 4), (1, 4, -1)):
        assert lib.mz_alpha_fill_workspace_bytes(*args, byref(out)) == INVALID, args
    assert lib.mz_alpha_fill_workspace_bytes(1, 4, 4, None) == INVALID
    assert lib.mz_alpha_fill_workspace_bytes(65535, 1 << 28, 1 << 28, byref(out)) == INVALID and "2^62" in lib.mz_last_error().decode()
    hw = (c_int * 8)()
    for args in ((0, 4, hw, 4), (4, 0, hw, 4), ((1 << 28) + 1, 4, hw, 4), (4, 4, hw, -1), (4, 4, None, 1)):
        assert lib.mz_debug_alpha_levels(*args) == INVALID, args[:2]


# ---- refusals of the C entries -----------------------------------------------------------------------------------------------------------
def ref(v):
    return byref(v) if v is not None else None


RGB_S, PLANE_S = (3 * H * W, H * W, W, 1), (H * W, 12345, W, 1)  # (the channel stride of a plane names nothing)
RGBA_S = (4 * H * W, 1, 4 * W, 4)                                 # interleaved HWC RGBA
HO, WO = R * H, R * W
RGB_O, PLANE_O = (3 * HO * WO, HO * WO, WO, 1), (HO * WO, 0, WO, 1)
RGBA_O = (4 * HO * WO, 1, 4 * WO, 4)
NEED = alpha_ref.workspace_bytes(B, H, W)


def fill(rgb="dense", alpha="dense", out="dense", elem=0, batch=B, h=H, w=W, premultiplied=0, ws=WS, ws_bytes=NEED):
    rgb = _ffi.view(FAKE, RGB_S) if rgb == "dense" else rgb
    alpha = _ffi.view(FAKE2, PLANE_S) if alpha == "dense" else alpha
    out = _ffi.view(FAKE3, RGB_S) if out == "dense" else out
    lib = _ffi.lib()
    code = lib.mz_alpha_fill(ref(rgb), ref(alpha), ref(out), elem, batch, h, w, premultiplied, ws, ws_bytes, None)
    return code, lib.mz_last_error().decode()


def merge(rgb="dense", alpha="dense", out_rgb="same", out_alpha="dense", elem=0, batch=B, hin=H, win=W, hout=HO, wout=WO, mode=2, premultiply=1):
    rgb = _ffi.view(FAKE, RGB_O) if rgb == "dense" else rgb
    out_rgb = rgb if out_rgb == "same" else out_rgb
    alpha = _ffi.view(FAKE2, PLANE_S) if alpha == "dense" else alpha
    out_alpha = _ffi.view(FAKE3, PLANE_O) if out_alpha == "dense" else out_alpha
    lib = _ffi.lib()
    code = lib.mz_alpha_merge(ref(rgb), ref(alpha), ref(out_rgb), ref(out_alpha), elem, batch, hin, win, hout, wout, mode, premultiply, None)
    return code, lib.mz_last_error().decode()


FILL_REFUSED = {
    "null rgb view": (dict(rgb=None), INVALID, "null"),
    "null alpha view": (dict(alpha=None), INVALID, "null"),
    "null out view": (dict(out=None), INVALID, "null"),
    "null rgb data": (dict(rgb=_ffi.view(None, RGB_S)), INVALID, "null data"),
    "null alpha data": (dict(alpha=_ffi.view(None, PLANE_S)), INVALID, "null data"),
    "null out data": (dict(out=_ffi.view(None, RGB_S)), INVALID, "null data"),
    "elem -1": (dict(elem=-1), INVALID, "elem"),
    "elem 4": (dict(elem=4), INVALID, "elem"),
    "no images": (dict(batch=0), INVALID, "B"),
    "65536 images": (dict(batch=65536), INVALID, "B"),
    "no rows": (dict(h=0), INVALID, "H, W"),
    "no columns": (dict(w=0), INVALID, "H, W"),
    "2^28 + 1 columns": (dict(w=(1 << 28) + 1), INVALID, "2^28"),
    "out row stride 0": (dict(out=_ffi.view(FAKE3, (3 * H * W, H * W, 0, 1))), INVALID, "row stride is 0"),
    "out channel stride 0": (dict(out=_ffi.view(FAKE3, (3 * H * W, 0, W, 1))), INVALID, "channel stride is 0"),
    "out column stride 0": (dict(out=_ffi.view(FAKE3, (3 * H * W, H * W, W, 0))), INVALID, "column stride is 0"),
    "out image stride 0 with two images": (dict(out=_ffi.view(FAKE3, (0, H * W, W, 1))), INVALID, "image stride is 0"),
    "out over rgb": (dict(out=_ffi.view(FAKE + 4, RGB_S)), INVALID, "rgb and out overlap"),
    "out is rgb": (dict(out=_ffi.view(FAKE, RGB_S)), INVALID, "rgb and out overlap"),
    "out over the last element of alpha": (dict(out=_ffi.view(FAKE2 + 4 * (B * H * W - 1), RGB_S)), INVALID, "alpha and out overlap"),
    "a byte range beyond 63 bits": (dict(rgb=_ffi.view(FAKE, (1 << 62, H * W, W, 1))), INVALID, "63 bits"),
    "null workspace": (dict(ws=None), TOO_SMALL, "workspace too small"),
    "workspace one byte short": (dict(ws_bytes=NEED - 1), TOO_SMALL, "workspace too small"),
    "no workspace bytes": (dict(ws_bytes=0), TOO_SMALL, "workspace too small"),
}
MERGE_REFUSED = {
    "null alpha view": (dict(alpha=None), "null"),
    "null out_alpha view": (dict(out_alpha=None), "null"),
    "null rgb view with premultiply": (dict(rgb=None, out_rgb=_ffi.view(FAKE, RGB_O)), "null"),
    "null out_rgb view with premultiply": (dict(out_rgb=None), "null"),
    "null alpha data": (dict(alpha=_ffi.view(None, PLANE_S)), "null data"),
    "null out_alpha data": (dict(out_alpha=_ffi.view(None, PLANE_O)), "null data"),
    "null rgb data": (dict(rgb=_ffi.view(None, RGB_O)), "null data"),
    "elem -1": (dict(elem=-1), "elem"),
    "elem 4": (dict(elem=4), "elem"),
    "no images": (dict(batch=0), "B"),
    "65536 images": (dict(batch=65536), "B"),
    "no input rows": (dict(hin=0), "sizes >= 1"),
    "no output columns": (dict(wout=0), "sizes >= 1"),
    "2^28 + 1 output rows": (dict(hout=(1 << 28) + 1), "2^28"),
    "mode -1": (dict(mode=-1), "mode"),
    "mode 3": (dict(mode=3), "mode"),
    "out_alpha row stride 0": (dict(out_alpha=_ffi.view(FAKE3, (HO * WO, 1, 0, 1))), "row stride is 0"),
    "out_alpha column stride 0": (dict(out_alpha=_ffi.view(FAKE3, (HO * WO, 1, WO, 0))), "column stride is 0"),
    "out_rgb channel stride 0": (dict(out_rgb=_ffi.view(FAKE, (3 * HO * WO, 0, WO, 1))), "channel stride is 0"),
    "out_alpha over alpha": (dict(out_alpha=_ffi.view(FAKE2 + 8, PLANE_O)), "alpha and out_alpha overlap"),
    "out_rgb over alpha": (dict(out_rgb=_ffi.view(FAKE2 - 16, RGB_O)), "alpha and out_rgb overlap"),
    "a byte range beyond 63 bits": (dict(out_alpha=_ffi.view(FAKE3, (1 << 62, 1, WO, 1))), "63 bits"),
}


@pytest.mark.parametrize("name", sorted(FILL_REFUSED))
def test_mz_alpha_fill_refuses(name):
    kw, want, word = FILL_REFUSED[name]
    code, msg = fill(**kw)
    assert code == want and word in msg, (name, code, msg)


@pytest.mark.parametrize("name", sorted(MERGE_REFUSED))
def test_mz_alpha_merge_refuses(name):
    kw, word = MERGE_REFUSED[name]
    code, msg = merge(**kw)
    assert code == INVALID and word in msg, (name, code, msg)


def test_layouts_that_are_accepted_pass_every_view_check():
    """each call stops at its LAST check -- the workspace of the fill, the mode of the merge -- so every view check has passed"""
    for elem in range(4):
        es = (4, 2, 2, 1)[elem]
        rgba = dict(rgb=_ffi.view(FAKE, RGBA_S), alpha=_ffi.view(FAKE + 3 * es, RGBA_S))  # one interleaved buffer, two views
        for kw in (dict(), rgba, dict(rgba, out=_ffi.view(FAKE3, RGBA_S)), dict(alpha=_ffi.view(FAKE2, (0, 0, 0, 0))), dict(premultiplied=1),
                   dict(rgb=_ffi.view(FAKE + 2 * es * H * W, (3 * H * W, -H * W, W, 1)))):  # (BGR: a negative channel stride)
            code, msg = fill(elem=elem, ws_bytes=NEED - 16, **kw)
            assert code == TOO_SMALL and "workspace too small" in msg, (elem, kw, code, msg)
        out = dict(rgb=_ffi.view(FAKE, RGBA_O), out_alpha=_ffi.view(FAKE + 3 * es, RGBA_O))       # in place in an interleaved result
        for kw in (dict(), out, dict(out, out_rgb=_ffi.view(FAKE3, RGB_O)), dict(premultiply=0, rgb=None, out_rgb=None),
                   dict(premultiply=0, rgb=None, out_rgb=None, out_alpha=_ffi.view(FAKE + 3 * es, RGBA_O))):
            code, msg = merge(elem=elem, mode=7, **kw)
            assert code == INVALID and "mode must be" in msg, (elem, kw, code, msg)


def test_declarations():
    header = (REPO / "include" / "mewzoom_hip.h").read_text()
    refusals = re.search(r"THE VIEW REFUSALS\..*?returns", header, re.S).group(0)
    assert "mz_alpha_fill" in refusals and "mz_alpha_merge" in refusals
    units = (REPO / "ultrazoom_amd" / "csrc" / "units.sh").read_text()
    assert re.search(r"kernel_units=\([^)]*\bmz_alpha\b", units)
    import ultrazoom_amd

    for name in ("alpha_fill", "alpha_merge", "upscale_rgba"):
        assert name in ultrazoom_amd.__all__ and callable(getattr(ultrazoom_amd, name))
    assert callable(ultrazoom_amd.MewZoom.upscale_rgba)
    for word in ("grey", "alpha through the model", "self-ensemble", "metrics with alpha"):  # what is out of scope is said
        assert word in " ".join(ultrazoom_amd.alpha.upscale_rgba.__doc__.split()), word


def test_python_refusals_come_from_shapes_and_dtypes_alone():
    from ultrazoom_amd import alpha_fill, alpha_merge, upscale_rgba

    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        alpha_fill(x[:, :3], x[:, 3:4])
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        alpha_fill(x, x[:, 3:4])
    with pytest.raises(ValueError, match="mode is"):
        alpha_merge(x[:, :3], x[:, 3:4], size=(4, 4), mode="area")
    with pytest.raises(ValueError, match=r"\[B, 4, H, W\]"):
        upscale_rgba(None, x[:, :3])


# ---- properties of the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(alpha_ref.DTYPES))
@pytest.mark.parametrize("h, w", [(9, 8), (17, 33), (1, 7), (5, 3)], ids=lambda v: str(v))
def test_the_restatement_reproduces_a_constant_exactly(h, w, dt):
    """binary alpha, one colour on the visible pixels: every pixel of the result is that colour, to the last bit"""
    x = alpha_ref.rgba(2, h, w, dt, kind="binary").clone()
    colour = torch.tensor([0.3, 0.6015625, 1.0], dtype=torch.float64)
    colour = (colour * 255 + 0.5).to(torch.uint8) if dt == "u8" else colour.to(alpha_ref.DTYPES[dt])
    x[:, :3] = colour.view(1, 3, 1, 1)
    noisy = alpha_ref.garbage(x, dt, "random")
    got = alpha_ref.fill_expected(noisy[:, :3], noisy[:, 3:4], dt, False)
    assert alpha_ref.same_bits(got, x[:, :3].contiguous())


@pytest.mark.parametrize("dt", sorted(alpha_ref.DTYPES))
@pytest.mark.parametrize("premultiplied", [False, True])
def test_a_fully_transparent_image_gives_zeros_and_no_nan(dt, premultiplied):
    for h, w in ((1, 1), (5, 3), (9, 8)):
        x = alpha_ref.garbage(alpha_ref.rgba(2, h, w, dt, kind="clear"), dt, "nan")
        got = alpha_ref.fill_expected(x[:, :3], x[:, 3:4], dt, premultiplied)
        assert alpha_ref.same_bits(got, torch.zeros_like(got))


@pytest.mark.parametrize("dt", sorted(alpha_ref.DTYPES))
@pytest.mark.parametrize("premultiplied", [False, True])
def test_the_colour_under_zero_alpha_is_never_read(dt, premultiplied):
    x = alpha_ref.rgba(2, 17, 33, dt)
    x = alpha_ref.premultiplied_of(x, dt) if premultiplied else x
    want = alpha_ref.fill_expected(x[:, :3], x[:, 3:4], dt, premultiplied)
    clear = torch.from_numpy(alpha_ref.alpha_values(x[:, 3:4]) == 0).expand(-1, 3, -1, -1)
    assert bool(clear.any()) and not bool(clear.all())
    for what in ("nan", "inf", "random"):
        g = alpha_ref.garbage(x, dt, what)
        assert not torch.equal(g[:, :3][clear], x[:, :3][clear]) or dt == "u8"
        assert alpha_ref.same_bits(alpha_ref.fill_expected(g[:, :3], g[:, 3:4], dt, premultiplied), want), what
    if not premultiplied:  # visible pixels come back as the bit patterns that went in
        assert alpha_ref.same_bits(want[~clear], x[:, :3][~clear])
    filled = color_ref.values(want)[clear.numpy()]
    assert np.isfinite(filled).all() and (filled >= 0).all() and (filled <= 1).all()


def test_an_opaque_image_comes_back_whole():
    for dt in sorted(alpha_ref.DTYPES):
        x = alpha_ref.rgba(2, 9, 8, dt, kind="opaque")
        assert alpha_ref.same_bits(alpha_ref.fill_expected(x[:, :3], x[:, 3:4], dt, False), x[:, :3].contiguous())


# ---- the weights that keep an opaque image opaque ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 4, 8])
def test_bicubic_weights_of_an_integer_ratio_sum_to_exactly_one(r):
    """interp_taps for bicubic at ratio r: interp_dot of the weights with ones -- acc = fma(w_k, 1, acc) from 0 in ascending k -- is exactly
    1.0 for every phase, in the library's weights and in the restatement's, so the alpha plane of an opaque image is exactly 1 (255)"""
    n_in = 9
    for i in range(n_in * r):
        for idx, w in (_ffi.interp_taps(n_in, n_in * r, 2, i), image_exact.interp_taps(n_in, n_in * r, "bicubic", i)[:2]):
            acc = 0.0
            for wk in w:
                acc = image_exact.fma_exact(float(wk), 1.0, acc)
            assert acc == 1.0 and len(w) == 4, (r, i, list(w), acc)
    ones = {dt: torch.ones((1, 1, 5, 7), dtype=alpha_ref.DTYPES[dt]) * (255 if dt == "u8" else 1) for dt in alpha_ref.DTYPES}
    for dt, a in ones.items():
        for mode in alpha_ref.MODES:
            got, _ = alpha_ref.merge_expected(None, a, (5 * r, 7 * r), mode, dt, False)
            assert alpha_ref.same_bits(got, torch.ones_like(got) * (255 if dt == "u8" else 1)), (dt, mode)
