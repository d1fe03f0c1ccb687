"""The 4:2:0 YCbCr entries without a GPU: the constants mz_debug_yuv_coeffs returns against tests/yuv_ref.py, the reference itself against
Pillow and against the luma reference, its round trip and its grey axis, every refused argument of mz_yuv420_to_rgb and mz_rgb_to_yuv420
(refused before anything touches a device) with the chroma-interleaving rule, the Python layer's refusals and the plane views of
nv12_planes / i420_planes."""

import struct
from ctypes import byref
from pathlib import Path

import numpy as np
import pytest
import torch

import color_ref
import yuv_ref
from ultrazoom_amd import _ffi
from yuv_ref import MATRIX_CODE, RANGE_CODE, SITINGS

REPO = Path(__file__).resolve().parent.parent
B, H, W = 2, 48, 64
HC, WC = H // 2, W // 2
DENSE3, DENSE1, DENSEC = (3 * H * W, H * W, W, 1), (H * W, H * W, W, 1), (HC * WC, HC * WC, WC, 1)
FAKE, FAKE2, FAR = 0x10000, 0x40000000, 0x70000000  # never dereferenced: validation comes first; far enough apart for any shape used here
INVALID = _ffi.MZ_ERR_INVALID_ARGUMENT
BAD_SITING = 2  # the codes are the entries' LAST check: a call refused for its siting has passed every check of its views, and nothing is launched


def bits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


# ---- the constants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", sorted(RANGE_CODE))
@pytest.mark.parametrize("matrix", sorted(MATRIX_CODE))
def test_the_library_compiles_the_constants_of_the_restatement(matrix, range_):
    got = _ffi.yuv_coeffs(MATRIX_CODE[matrix], RANGE_CODE[range_])
    want = yuv_ref.debug_coeffs(matrix, range_)
    assert [bits(v) for v in got] == [bits(v) for v in want], (got, want)
    k = yuv_ref.coeffs(matrix, range_)
    assert abs(k["kr"] + k["kg"] + k["kb"] - 1.0) < 1e-15 and k["g_r"] < 0 and k["g_b"] < 0


def test_the_coefficient_entry_refuses_bad_arguments():
    lib = _ffi.lib()
    out = (_ffi.c_double * 9)()
    assert lib.mz_debug_yuv_coeffs(0, 0, None) == INVALID
    for m, r in [(-1, 0), (2, 0), (0, -1), (0, 2)]:
        assert lib.mz_debug_yuv_coeffs(m, r, out) == INVALID, (m, r)


def test_declarations():
    import ultrazoom_amd

    assert "mz_yuv" in (REPO / "ultrazoom_amd" / "csrc" / "units.sh").read_text()
    for name in ("yuv420_to_rgb", "rgb_to_yuv420", "nv12_planes", "i420_planes"):
        assert name in ultrazoom_amd.__all__ and getattr(ultrazoom_amd, name) is getattr(ultrazoom_amd.video, name)
    assert callable(ultrazoom_amd.MewZoom.upscale_yuv420)


# ---- the restatement against other statements of the same standards ----------------------------------------------------------------------
def colours(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.int64).to(torch.uint8).numpy()


def test_per_pixel_functions_agree_with_pillow_to_one_code():
    """Pillow's "YCbCr" is JFIF: BT.601, full range, in fixed point.  Both directions, all six channels: at most 1 code value apart."""
    from PIL import Image

    k = yuv_ref.coeffs("bt601", "full")
    c = colours(257, 263, 1)
    want = np.asarray(Image.fromarray(c, "RGB").convert("YCbCr")).astype(np.int64)
    v = c.astype(np.float64) / 255.0
    y, pb, pr = yuv_ref.yuv_pixel(k, v[..., 0], v[..., 1], v[..., 2])
    got = np.stack([yuv_ref.code(k["sy"], y, k["yoff"]), yuv_ref.code(k["sc"], pb, 128.0), yuv_ref.code(k["sc"], pr, 128.0)], axis=-1).astype(np.int64)
    diff = np.abs(got - want).reshape(-1, 3).max(axis=0)
    print("RGB -> YCbCr, max code difference per channel:", diff)
    assert (diff <= 1).all(), diff
    c = colours(257, 263, 2)  # now read as (Y, Cb, Cr)
    want = np.asarray(Image.fromarray(c, "YCbCr").convert("RGB")).astype(np.int64)
    rgb = np.stack(yuv_ref.rgb_pixel(k, c[..., 0], c[..., 1].astype(np.float64), c[..., 2].astype(np.float64)), axis=-1)
    got = color_ref.store(rgb, "u8", 1).numpy().astype(np.int64)
    diff = np.abs(got - want).reshape(-1, 3).max(axis=0)
    print("YCbCr -> RGB, max code difference per channel:", diff)
    assert (diff <= 1).all(), diff


@pytest.mark.parametrize("range_, standard", [("limited", "bt601"), ("full", "full")])
def test_y_codes_agree_with_the_luma_reference_to_one_code(range_, standard):
    """BT.601 Y of a uint8 colour, two statements: this one (Kr r + Kg g + Kb b, then Sy y + Yoff) and mz_color.h's (the constants of
    MATLAB's rgb2ycbcr / JFIF); on random colours and on every colour at which the luma reference's rounding is a tie"""
    k = yuv_ref.coeffs("bt601", range_)
    rnd = colours(256, 256, 3).reshape(-1, 3)
    for c in (rnd, color_ref.u8_ties("bt601"), color_ref.u8_ties("full")):
        x = torch.from_numpy(np.ascontiguousarray(c.T).reshape(1, 3, 1, -1))
        want = color_ref.luma_expected(x, standard, "u8", 0).numpy().astype(np.int64)
        v = color_ref.values(x)
        y, _, _ = yuv_ref.yuv_pixel(k, v[:, 0:1], v[:, 1:2], v[:, 2:3])
        got = yuv_ref.code(k["sy"], y, k["yoff"]).astype(np.int64)
        assert got.shape == want.shape and int(np.abs(got - want).max()) <= 1


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("range_", sorted(RANGE_CODE))
@pytest.mark.parametrize("matrix", sorted(MATRIX_CODE))
def test_round_trip_of_the_restatement_returns_the_planes(matrix, range_, siting):
    """random Y, chroma constant per image -> unclamped float32 RGB -> planes: exactly the planes (such frames are out of gamut, hence no
    clamp; a constant survives both chroma filters exactly, and float32 keeps far more than the 8 bits of a code)"""
    for h, w in [(1, 1), (2, 2), (3, 5), (17, 33), (64, 130)]:
        y, cb, cr = yuv_ref.grey_chroma_frames(2, h, w)
        rgb = yuv_ref.to_rgb_expected(y, cb, cr, matrix, range_, siting, "f32", 0)
        back = yuv_ref.to_yuv_expected(rgb, matrix, range_, siting)
        for name, got, want in zip("y cb cr".split(), back, (y, cb, cr)):
            assert torch.equal(got, want), (h, w, name)


@pytest.mark.parametrize("range_", sorted(RANGE_CODE))
@pytest.mark.parametrize("matrix", sorted(MATRIX_CODE))
def test_grey_frames_have_equal_channels_bit_for_bit(matrix, range_):
    y = torch.arange(256, dtype=torch.int64).to(torch.uint8).reshape(1, 1, 16, 16)
    c = torch.full((1, 1, 8, 8), 128, dtype=torch.uint8)
    for siting in SITINGS:
        rgb = yuv_ref.to_rgb_f64(y, c, c, matrix, range_, siting)
        assert np.array_equal(rgb[:, 0].view(np.int64), rgb[:, 1].view(np.int64)) and np.array_equal(rgb[:, 0].view(np.int64), rgb[:, 2].view(np.int64))


def test_the_filters_of_the_restatement():
    """by hand: the taps at the edges and in the middle of a 4-sample row / column"""
    c = np.array([[[[0.0, 16.0, 32.0, 48.0]]]])
    left = yuv_ref.chroma_up(c, 1, 8, "left")[0, 0, 0]
    assert left.tolist() == [0.0, 8.0, 16.0, 24.0, 32.0, 40.0, 48.0, 48.0]
    center = yuv_ref.chroma_up(c, 1, 8, "center")[0, 0, 0]
    assert center.tolist() == [0.0, 4.0, 12.0, 20.0, 28.0, 36.0, 44.0, 48.0]
    col = yuv_ref.chroma_up(c.reshape(1, 1, 4, 1), 7, 1, "left")[0, 0, :, 0]  # odd height: row 6 is the even row of sample 3
    assert col.tolist() == [0.0, 4.0, 12.0, 20.0, 28.0, 36.0, 44.0]
    p = np.arange(10.0).reshape(1, 1, 2, 5)  # rows 0..4 and 5..9: u = 2.5 .. 6.5
    assert yuv_ref.chroma_down(p, "center")[0, 0].tolist() == [[3.0, 5.0, 6.5]]
    assert yuv_ref.chroma_down(p, "left")[0, 0].tolist() == [[2.75, 4.5, 6.25]]


# ---- refusals of the C entries -------------------------------------------------------------------------------------------------------------
def ref(v):
    return byref(v) if v is not None else None


def to_rgb(y="dense", cb="dense", cr="dense", out="dense", elem=0, batch=B, h=H, w=W, matrix=1, range_=0, siting=0):
    y = _ffi.view(FAKE, DENSE1) if y == "dense" else y
    cb = _ffi.view(FAKE + B * H * W, DENSEC) if cb == "dense" else cb
    cr = _ffi.view(FAKE + B * H * W + B * HC * WC, DENSEC) if cr == "dense" else cr
    out = _ffi.view(FAKE2, DENSE3) if out == "dense" else out
    lib = _ffi.lib()
    code = lib.mz_yuv420_to_rgb(ref(y), ref(cb), ref(cr), ref(out), elem, batch, h, w, matrix, range_, siting, 1, None)
    return code, lib.mz_last_error().decode()


def to_yuv(x="dense", y="dense", cb="dense", cr="dense", elem=0, batch=B, h=H, w=W, matrix=1, range_=0, siting=0):
    x = _ffi.view(FAKE2, DENSE3) if x == "dense" else x
    y = _ffi.view(FAKE, DENSE1) if y == "dense" else y
    cb = _ffi.view(FAKE + B * H * W, DENSEC) if cb == "dense" else cb
    cr = _ffi.view(FAKE + B * H * W + B * HC * WC, DENSEC) if cr == "dense" else cr
    lib = _ffi.lib()
    code = lib.mz_rgb_to_yuv420(ref(x), elem, ref(y), ref(cb), ref(cr), batch, h, w, matrix, range_, siting, None)
    return code, lib.mz_last_error().decode()


SHARED_REFUSED = {
    "null y view": (dict(y=None), "null"),
    "null cb view": (dict(cb=None), "null"),
    "null cr view": (dict(cr=None), "null"),
    "null y data": (dict(y=_ffi.view(None, DENSE1)), "null data"),
    "null cb data": (dict(cb=_ffi.view(None, DENSEC)), "null data"),
    "null cr data": (dict(cr=_ffi.view(None, DENSEC)), "null data"),
    "elem -1": (dict(elem=-1), "elem"),
    "elem 4": (dict(elem=4), "elem"),
    "matrix -1": (dict(matrix=-1), "matrix"),
    "matrix 2": (dict(matrix=2), "matrix"),
    "range 2": (dict(range_=2), "range"),
    "range -1": (dict(range_=-1), "range"),
    "siting 2": (dict(siting=2), "siting"),
    "siting -1": (dict(siting=-1), "siting"),
    "no images": (dict(batch=0), "B"),
    "65536 images": (dict(batch=65536), "B"),
    "no rows": (dict(h=0), "H, W"),
    "no columns": (dict(w=0), "H, W"),
    "2^28 + 1 columns": (dict(w=(1 << 28) + 1), "2^28"),
}
TO_RGB_REFUSED = dict(SHARED_REFUSED, **{
    "null out view": (dict(out=None), "null"),
    "null out data": (dict(out=_ffi.view(None, DENSE3)), "null data"),
    "out row stride 0": (dict(out=_ffi.view(FAKE2, (3 * H * W, H * W, 0, 1))), "row stride is 0"),
    "out channel stride 0": (dict(out=_ffi.view(FAKE2, (3 * H * W, 0, W, 1))), "channel stride is 0"),
    "out over y": (dict(out=_ffi.view(FAKE, DENSE3)), "Y plane overlap"),
    "out over cb": (dict(y=_ffi.view(FAR, DENSE1), out=_ffi.view(FAKE + B * H * W, DENSE3)), "Cb plane overlap"),
    "out over cr": (dict(y=_ffi.view(FAR, DENSE1), cb=_ffi.view(FAR + B * H * W, DENSEC), out=_ffi.view(FAKE + B * H * W + B * HC * WC, DENSE3)),
                    "Cr plane overlap"),
    "a byte range beyond 63 bits": (dict(out=_ffi.view(FAKE2, (1 << 62, H * W, W, 1))), "63 bits"),
})
TO_YUV_REFUSED = dict(SHARED_REFUSED, **{
    "null x view": (dict(x=None), "null"),
    "null x data": (dict(x=_ffi.view(None, DENSE3)), "null data"),
    "y row stride 0": (dict(y=_ffi.view(FAKE, (H * W, 1, 0, 1))), "row stride is 0"),
    "cb column stride 0": (dict(cb=_ffi.view(FAKE + B * H * W, (HC * WC, 1, WC, 0))), "column stride is 0"),
    "cr image stride 0 with two images": (dict(cr=_ffi.view(FAKE + B * H * W + B * HC * WC, (0, 1, WC, 1))), "image stride is 0"),
    "x over y": (dict(x=_ffi.view(FAKE, DENSE3)), "Y plane overlap"),
    "x over cr": (dict(x=_ffi.view(FAKE + B * H * W + 2 * B * HC * WC - 1, DENSE3)), "Cr plane overlap"),
    "y over cb": (dict(y=_ffi.view(FAKE + 1, DENSE1)), "Y plane and a chroma plane overlap"),
    "cr is cb": (dict(cr=_ffi.view(FAKE + B * H * W, DENSEC)), "Cb and Cr planes overlap"),
    "cr one byte behind a planar cb": (dict(cr=_ffi.view(FAKE + B * H * W + 1, DENSEC)), "Cb and Cr planes overlap"),
    "cr one row behind cb": (dict(cr=_ffi.view(FAKE + B * H * W + WC, DENSEC)), "Cb and Cr planes overlap"),
})


@pytest.mark.parametrize("name", sorted(TO_RGB_REFUSED))
def test_mz_yuv420_to_rgb_refuses(name):
    kw, word = TO_RGB_REFUSED[name]
    code, msg = to_rgb(**kw)
    assert code == INVALID and word in msg, (name, code, msg)


@pytest.mark.parametrize("name", sorted(TO_YUV_REFUSED))
def test_mz_rgb_to_yuv420_refuses(name):
    kw, word = TO_YUV_REFUSED[name]
    code, msg = to_yuv(**kw)
    assert code == INVALID and word in msg, (name, code, msg)


# frame buffers at FAKE: [B, H * 3 / 2, W] bytes, the chroma of a frame H * W bytes behind its Y
FRAME = H * W * 3 // 2
Y_OF_FRAMES = (FRAME, 1, W, 1)
PAIRS = (FRAME, 1, W, 2)          # NV12 / NV21: a row of W / 2 pairs
PLANAR = (FRAME, 1, WC, 1)        # I420 / YV12
WIDE = (4 * HC * WC, 1, 4 * WC, 4)  # four interleaved planes: a column stride of 4


def chroma_case(cb_at, cr_at, strides, cr_strides=None, frames=False):
    """Cb and Cr in the chroma part of the frame buffers; Y in front of them (frames: the four containers) or dense and far away"""
    return dict(y=_ffi.view(FAKE, Y_OF_FRAMES) if frames else _ffi.view(FAR, DENSE1), cb=_ffi.view(FAKE + H * W + cb_at, strides), cr=_ffi.view(FAKE + H * W + cr_at, cr_strides or strides))


CHROMA_ACCEPTED = {
    "dense planes": {},
    "nv12": chroma_case(0, 1, PAIRS, frames=True),
    "nv21": chroma_case(1, 0, PAIRS, frames=True),
    "i420": chroma_case(0, HC * WC, PLANAR, frames=True),
    "yv12": chroma_case(HC * WC, 0, PLANAR, frames=True),
    "column stride 4, three bytes apart": chroma_case(0, 3, WIDE),
    "column stride 4, three bytes behind": chroma_case(3, 0, WIDE),
}
CHROMA_REFUSED = {
    "the same interleaved view twice": chroma_case(0, 0, PAIRS),
    "a whole pair apart": chroma_case(0, 2, PAIRS),
    "column stride 4, four bytes apart": chroma_case(0, 4, WIDE),
    "interleaved bases, different row strides": chroma_case(0, 1, PAIRS, (FRAME, 1, 2 * W, 2)),
    "interleaved bases, different image strides": chroma_case(0, 1, PAIRS, (2 * FRAME, 1, W, 2)),
    "one byte apart with column stride 1": chroma_case(0, 1, PLANAR),
    "planar, half a plane apart": chroma_case(0, HC * WC // 2, PLANAR),
    "negative column stride -2, one byte apart": chroma_case(W - 2, W - 1, (FRAME, 1, W, -2)),
}


@pytest.mark.parametrize("name", sorted(CHROMA_ACCEPTED))
def test_chroma_layouts_that_are_accepted_pass_every_view_check(name):
    code, msg = to_yuv(siting=BAD_SITING, **CHROMA_ACCEPTED[name])
    assert code == INVALID and "siting must be" in msg, (name, code, msg)


@pytest.mark.parametrize("name", sorted(CHROMA_REFUSED))
def test_chroma_views_that_alias_are_refused(name):
    code, msg = to_yuv(**CHROMA_REFUSED[name])
    assert code == INVALID and "Cb and Cr planes overlap" in msg, (name, code, msg)


def test_planes_that_only_read_may_alias_each_other():
    """mz_yuv420_to_rgb reads its planes: Cb and Cr may be one view (a grey-chroma frame), whatever their layout"""
    same = _ffi.view(FAKE + B * H * W, DENSEC)
    code, msg = to_rgb(cb=same, cr=same, siting=BAD_SITING)
    assert code == INVALID and "siting must be" in msg, (code, msg)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_plane_views_of_frame_buffers():
    from ultrazoom_amd import i420_planes, nv12_planes

    b, h, w = 2, 8, 12
    buf = torch.arange(b * h * 3 // 2 * w, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(b, h * 3 // 2, w)
    flat = buf.reshape(b, -1)
    y, cb, cr = nv12_planes(buf)
    assert y.shape == (b, 1, h, w) and cb.shape == cr.shape == (b, 1, h // 2, w // 2)
    assert torch.equal(y[:, 0], buf[:, :h]) and torch.equal(cb.reshape(b, -1), flat[:, h * w::2]) and torch.equal(cr.reshape(b, -1), flat[:, h * w + 1::2])
    y2, cr2, cb2 = nv12_planes(buf, order="vu")
    assert cb2.data_ptr() == cb.data_ptr() and cr2.data_ptr() == cr.data_ptr() and cb2.stride() == cb.stride()
    y, cb, cr = i420_planes(buf)
    q = h * w // 4
    assert cb.shape == cr.shape == (b, 1, h // 2, w // 2)
    assert torch.equal(cb.reshape(b, -1), flat[:, h * w:h * w + q]) and torch.equal(cr.reshape(b, -1), flat[:, h * w + q:])
    y2, cr2, cb2 = i420_planes(buf, order="vu")
    assert cb2.data_ptr() == cb.data_ptr() and cr2.data_ptr() == cr.data_ptr()
    for t in (y, cb, cr):  # views: nothing is copied
        assert t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    wide = torch.zeros(b, h * 3 // 2, 2 * w, dtype=torch.uint8)[:, :, :w]  # rows of a wider buffer: NV12 views exist, I420's do not
    assert nv12_planes(wide)[1].stride() == (h * 3 // 2 * 2 * w, h // 2 * 2 * w, 2 * w, 2)
    with pytest.raises(ValueError, match="dense"):
        i420_planes(wide)
    for bad in (torch.zeros(2, 12, 7, dtype=torch.uint8), torch.zeros(2, 10, 8, dtype=torch.uint8), torch.zeros(2, 11, 8, dtype=torch.uint8),
                torch.zeros(12, 8, dtype=torch.uint8), torch.zeros(2, 12, 8)):
        for fn in (nv12_planes, i420_planes):
            with pytest.raises(ValueError):
                fn(bad)
    with pytest.raises(ValueError, match="order"):
        nv12_planes(buf, order="yuv")


def test_python_refusals_come_from_shapes_and_dtypes_alone():
    """on CPU tensors: a ValueError for every wrong shape, dtype or name, before the device is looked at; right arguments reach the
    'no CPU path' error"""
    from ultrazoom_amd import rgb_to_yuv420, yuv420_to_rgb

    y, c = torch.zeros(2, 1, 5, 7, dtype=torch.uint8), torch.zeros(2, 1, 3, 4, dtype=torch.uint8)
    for kw in (dict(matrix="bt2020"), dict(range="tv"), dict(siting="top"), dict(dtype=torch.float64), dict(out=torch.zeros(2, 3, 5, 8))):
        with pytest.raises(ValueError):
            yuv420_to_rgb(y, c, c, **kw)
    for args in ((y[:, 0], c, c), (y, c[..., :3], c), (y, c, c[:, :, :2]), (y.float(), c, c), (y, c, c.to(torch.int8)), (y[:0], c[:0], c[:0])):
        with pytest.raises(ValueError):
            yuv420_to_rgb(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        yuv420_to_rgb(y, c, c)
    x = torch.zeros(2, 3, 5, 7)
    for kw in (dict(matrix=0), dict(range="limited "), dict(siting=None), dict(out=(y, c)), dict(out=(y, c, c[..., :3])), dict(out=(y.float(), c, c)),
               dict(out=(y[..., :6], c, c))):
        with pytest.raises(ValueError):
            rgb_to_yuv420(x, **kw)
    for bad in (x[:, :2], x[0], x.double(), x[:, :, :0]):
        with pytest.raises(ValueError):
            rgb_to_yuv420(bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rgb_to_yuv420(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rgb_to_yuv420(x, out=(y, c, c))
