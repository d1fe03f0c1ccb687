"""The YCbCr entries of any depth and subsampling without a GPU: the constants mz_debug_ycbcr_coeffs returns against tests/ycbcr_ref.py and
against mz_debug_yuv_coeffs, the restatement against tests/yuv_ref.py at depth 8 and 4:2:0, its round trip at every depth, its filters
and alignments by hand, every refused argument of mz_ycbcr_to_rgb and mz_rgb_to_ycbcr (refused before anything touches a device) with
the chroma-interleaving rule in elements, the Python layer's refusals and the plane views of frame_planes."""

import itertools
import struct
from ctypes import byref
from pathlib import Path

import numpy as np
import pytest
import torch

import color_ref
import ycbcr_ref
import yuv_ref
from ultrazoom_amd import _ffi
from ycbcr_ref import ALIGNS, DEPTHS, MATRIX_CODE, RANGE_CODE, SITINGS, SUBSAMPLINGS

REPO = Path(__file__).resolve().parent.parent
B, H, W = 2, 48, 64
FAKE, FAKE2, FAR = 0x10000, 0x40000000, 0x70000000  # never dereferenced: validation comes first
INVALID = _ffi.MZ_ERR_INVALID_ARGUMENT
BAD_SITING = 2  # the codes are the entries' LAST check: a call refused for its siting has passed every check of its views


def bits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


# ---- the constants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("range_", sorted(RANGE_CODE))
@pytest.mark.parametrize("matrix", sorted(MATRIX_CODE))
def test_the_library_compiles_the_constants_of_the_restatement(matrix, range_, depth):
    got = _ffi.ycbcr_coeffs(MATRIX_CODE[matrix], RANGE_CODE[range_], depth)
    want = ycbcr_ref.debug_coeffs(matrix, range_, depth)
    assert len(got) == 11 and [bits(v) for v in got] == [bits(v) for v in want], (got, want)
    assert got[9] == 2.0 ** (depth - 1) and got[10] == 2.0 ** depth - 1
    if depth == 8 and matrix != "bt2020":
        old = _ffi.yuv_coeffs(MATRIX_CODE[matrix], RANGE_CODE[range_])
        assert [bits(v) for v in got[:9]] == [bits(v) for v in old]


def test_bt2020_has_the_coefficients_of_the_standard():
    got = _ffi.ycbcr_coeffs(2, 0, 10)
    assert abs(got[3] - 1.4746) < 1e-15 and abs(got[4] - 1.8814) < 1e-15, got  # a_r, a_b
    k = ycbcr_ref.coeffs("bt2020", "limited", 10)
    assert abs(k["kr"] + k["kg"] + k["kb"] - 1.0) < 1e-15 and k["g_r"] < 0 and k["g_b"] < 0


def test_the_coefficient_entries_refuse_bad_arguments():
    lib = _ffi.lib()
    out = (_ffi.c_double * 11)()
    assert lib.mz_debug_ycbcr_coeffs(0, 0, 8, None) == INVALID
    for m, r, d in [(-1, 0, 8), (3, 0, 8), (0, -1, 8), (0, 2, 8), (0, 0, 9), (0, 0, 0), (0, 0, 14), (0, 0, 32)]:
        assert lib.mz_debug_ycbcr_coeffs(m, r, d, out) == INVALID, (m, r, d)
    assert lib.mz_debug_yuv_coeffs(2, 0, (_ffi.c_double * 9)()) == INVALID  # the 4:2:0 entries keep refusing bt2020


def test_declarations():
    import ultrazoom_amd

    assert "mz_ycbcr" in (REPO / "ultrazoom_amd" / "csrc" / "units.sh").read_text()
    for name in ("ycbcr_to_rgb", "rgb_to_ycbcr", "frame_planes"):
        assert name in ultrazoom_amd.__all__ and getattr(ultrazoom_amd, name) is getattr(ultrazoom_amd.video, name)
    assert callable(ultrazoom_amd.MewZoom.upscale_ycbcr)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", yuv_ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_restatement_at_depth_8_and_420_is_the_restatement_of_the_420_entries(shape):
    h, w = shape
    planes = yuv_ref.planes(2, h, w)
    for matrix, range_, siting in itertools.product(sorted(yuv_ref.MATRIX_CODE), sorted(RANGE_CODE), SITINGS):
        for align in ALIGNS:
            got = ycbcr_ref.to_rgb_f64(*planes, 8, align, "420", matrix, range_, siting)
            want = yuv_ref.to_rgb_f64(*planes, matrix, range_, siting)
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (matrix, range_, siting)
            for dt in sorted(color_ref.DTYPES):
                x = color_ref.image(2, h, w, dt)
                for g, wnt in zip(ycbcr_ref.to_ycbcr_expected(x, 8, align, "420", matrix, range_, siting), yuv_ref.to_yuv_expected(x, matrix, range_, siting)):
                    assert g.dtype == np.uint8 and np.array_equal(g, wnt.numpy()), (matrix, range_, siting, dt)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("range_", sorted(RANGE_CODE))
@pytest.mark.parametrize("matrix", sorted(MATRIX_CODE))
def test_round_trip_of_the_restatement_returns_the_planes(matrix, range_, depth):
    """random Y, chroma constant per image -> unclamped float32 RGB -> planes: exactly the planes, 16 bits included (float32 only: float16
    loses codes above 10 bits, bfloat16 at every depth)"""
    n = 0
    for (h, w), sub, siting, align in itertools.product([(1, 1), (3, 5), (17, 33)], SUBSAMPLINGS, SITINGS, ALIGNS):
        if n % 3 != (h + len(sub) + len(siting)) % 3 and (h, w) != (3, 5):  # every subsampling, siting and align, a third of the products
            n += 1
            continue
        n += 1
        planes = ycbcr_ref.grey_chroma_frames(2, h, w, depth, align, sub)
        rgb = ycbcr_ref.to_rgb_expected(*planes, depth, align, sub, matrix, range_, siting, "f32", 0)
        back = ycbcr_ref.to_ycbcr_expected(rgb, depth, align, sub, matrix, range_, siting)
        for name, got, want in zip("y cb cr".split(), back, planes):
            assert got.dtype == want.dtype and np.array_equal(got, want), (h, w, sub, siting, align, name)


def test_the_filters_of_422_and_444_by_hand():
    c = np.array([[[[0.0, 16.0, 32.0, 48.0], [64.0, 80.0, 96.0, 112.0]]]])  # two rows: no row reaches the other
    left = ycbcr_ref.chroma_up(c, 2, 8, "left", "422")[0, 0]
    assert left[0].tolist() == [0.0, 8.0, 16.0, 24.0, 32.0, 40.0, 48.0, 48.0] and left[1].tolist() == [64.0, 72.0, 80.0, 88.0, 96.0, 104.0, 112.0, 112.0]
    center = ycbcr_ref.chroma_up(c, 2, 8, "center", "422")[0, 0]
    assert center[0].tolist() == [0.0, 4.0, 12.0, 20.0, 28.0, 36.0, 44.0, 48.0]
    odd = ycbcr_ref.chroma_up(c, 2, 7, "left", "422")[0, 0]  # odd width: column 6 is the even column of sample 3
    assert odd[0].tolist() == [0.0, 8.0, 16.0, 24.0, 32.0, 40.0, 48.0]
    for siting in SITINGS:
        assert np.array_equal(ycbcr_ref.chroma_up(c, 2, 4, siting, "444"), c)
    p = np.arange(10.0).reshape(1, 1, 2, 5)
    assert ycbcr_ref.chroma_down(p, "center", "422")[0, 0].tolist() == [[0.5, 2.5, 4.0], [5.5, 7.5, 9.0]]
    assert ycbcr_ref.chroma_down(p, "left", "422")[0, 0].tolist() == [[0.25, 2.0, 3.75], [5.25, 7.0, 8.75]]
    for siting in SITINGS:
        assert np.array_equal(ycbcr_ref.chroma_down(p, siting, "444"), p)
    assert ycbcr_ref.chroma_hw(5, 7, "420") == (3, 4) and ycbcr_ref.chroma_hw(5, 7, "422") == (5, 4) and ycbcr_ref.chroma_hw(5, 7, "444") == (5, 7)


@pytest.mark.parametrize("depth", (10, 12))
def test_bits_outside_the_code_do_not_change_the_rgb(depth):
    """"high" ignores the low 16 - d bits of a word, "low" the high ones"""
    h, w, sub = 5, 9, "420"
    codes = [ycbcr_ref.read(p, depth, "low") for p in ycbcr_ref.planes(2, h, w, depth, sub)]
    rng = np.random.default_rng(5)
    for align in ALIGNS:
        clean = [ycbcr_ref.write(c, depth, align) for c in codes]
        junk = [rng.integers(0, 2 ** (16 - depth), size=c.shape) for c in codes]
        dirty = [(c.astype(np.int64) | (j if align == "high" else j << depth)).astype(np.uint16) for c, j in zip(clean, junk)]
        assert any((d != c).any() for d, c in zip(dirty, clean))
        a = ycbcr_ref.to_rgb_f64(*clean, depth, align, sub, "bt2020", "limited", "left")
        b = ycbcr_ref.to_rgb_f64(*dirty, depth, align, sub, "bt2020", "limited", "left")
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert all((ycbcr_ref.read(c, depth, align) == k).all() for c, k in zip(clean, codes))
    assert (ycbcr_ref.write(codes[0], depth, "high") & (2 ** (16 - depth) - 1) == 0).all()  # a high-aligned word's low bits are zero


# ---- refusals of the C entries -------------------------------------------------------------------------------------------------------------
def ref(v):
    return byref(v) if v is not None else None


def layout(depth=10, sub=0):
    """dense planes at FAKE for a B x H x W frame: (element bytes, Hc, Wc, y strides, chroma strides, Cb address, Cr address)"""
    es = 2 if depth > 8 else 1
    hc, wc = (H // 2 if sub == 0 else H), (W if sub == 2 else W // 2)
    return es, hc, wc, (H * W, 1, W, 1), (hc * wc, 1, wc, 1), FAKE + es * B * H * W, FAKE + es * (B * H * W + B * hc * wc)


DENSE3 = (3 * H * W, H * W, W, 1)


def call(direction, y="dense", cb="dense", cr="dense", rgb="dense", elem=0, batch=B, h=H, w=W, depth=10, align=0, sub=0, matrix=2, range_=0, siting=0):
    es, hc, wc, ys, cs, cb_at, cr_at = layout(depth if depth in DEPTHS else 10, sub if sub in (0, 1, 2) else 0)
    y = _ffi.view(FAKE, ys) if y == "dense" else y
    cb = _ffi.view(cb_at, cs) if cb == "dense" else cb
    cr = _ffi.view(cr_at, cs) if cr == "dense" else cr
    rgb = _ffi.view(FAKE2, DENSE3) if rgb == "dense" else rgb
    lib = _ffi.lib()
    if direction == "to_rgb":
        code = lib.mz_ycbcr_to_rgb(ref(y), ref(cb), ref(cr), depth, align, sub, ref(rgb), elem, batch, h, w, matrix, range_, siting, 1, None)
    else:
        code = lib.mz_rgb_to_ycbcr(ref(rgb), elem, ref(y), ref(cb), ref(cr), depth, align, sub, batch, h, w, matrix, range_, siting, None)
    return code, lib.mz_last_error().decode()


_, HC, WC, YS, CS, CB_AT, CR_AT = layout()
SHARED_REFUSED = {
    "null y view": (dict(y=None), "null"),
    "null cb view": (dict(cb=None), "null"),
    "null cr view": (dict(cr=None), "null"),
    "null rgb view": (dict(rgb=None), "null"),
    "null y data": (dict(y=_ffi.view(None, YS)), "null data"),
    "null cb data": (dict(cb=_ffi.view(None, CS)), "null data"),
    "null cr data": (dict(cr=_ffi.view(None, CS)), "null data"),
    "null rgb data": (dict(rgb=_ffi.view(None, DENSE3)), "null data"),
    "elem -1": (dict(elem=-1), "elem"),
    "elem 4": (dict(elem=4), "elem"),
    "depth 9": (dict(depth=9), "depth"),
    "depth 0": (dict(depth=0), "depth"),
    "depth 14": (dict(depth=14), "depth"),
    "depth 32": (dict(depth=32), "depth"),
    "align -1": (dict(align=-1), "align"),
    "align 2": (dict(align=2), "align"),
    "subsampling -1": (dict(sub=-1), "subsampling"),
    "subsampling 3": (dict(sub=3), "subsampling"),
    "matrix -1": (dict(matrix=-1), "matrix"),
    "matrix 3": (dict(matrix=3), "matrix"),
    "range 2": (dict(range_=2), "range"),
    "range -1": (dict(range_=-1), "range"),
    "siting 2": (dict(siting=2), "siting"),
    "siting -1": (dict(siting=-1), "siting"),
    "no images": (dict(batch=0), "B"),
    "65536 images": (dict(batch=65536), "B"),
    "no rows": (dict(h=0), "H, W"),
    "no columns": (dict(w=0), "H, W"),
    "2^28 + 1 columns": (dict(w=(1 << 28) + 1), "2^28"),
    "y at an odd address, depth 10": (dict(y=_ffi.view(FAR + 1, YS)), "aligned to 2 bytes"),
    "cb at an odd address, depth 16": (dict(depth=16, cb=_ffi.view(FAR + 1, CS)), "aligned to 2 bytes"),
    "cr at an odd address, depth 12": (dict(depth=12, cr=_ffi.view(FAR + 1, CS)), "aligned to 2 bytes"),
    # 16-bit elements: the RGB view begins inside the second HALF of the Y plane's bytes, past where 8-bit planes of these strides would end
    "rgb over the second half of a 16-bit y": (dict(rgb=_ffi.view(FAKE + B * H * W + 64, DENSE3), cb=_ffi.view(FAR, CS), cr=_ffi.view(FAR + 0x100000, CS)),
                                               "Y plane overlap"),
    "rgb over cb": (dict(y=_ffi.view(FAR, YS), rgb=_ffi.view(CB_AT, DENSE3)), "Cb plane overlap"),
    "rgb over the last element of cr": (dict(y=_ffi.view(FAR, YS), cb=_ffi.view(FAR + 0x100000, CS), rgb=_ffi.view(CR_AT + 2 * B * HC * WC - 2, DENSE3)),
                                        "Cr plane overlap"),
    "a byte range beyond 63 bits": (dict(rgb=_ffi.view(FAKE2, (1 << 62, H * W, W, 1))), "63 bits"),
}
TO_RGB_REFUSED = dict(SHARED_REFUSED, **{
    "out row stride 0": (dict(rgb=_ffi.view(FAKE2, (3 * H * W, H * W, 0, 1))), "row stride is 0"),
    "out channel stride 0": (dict(rgb=_ffi.view(FAKE2, (3 * H * W, 0, W, 1))), "channel stride is 0"),
})
TO_YCBCR_REFUSED = dict(SHARED_REFUSED, **{
    "y row stride 0": (dict(y=_ffi.view(FAKE, (H * W, 1, 0, 1))), "row stride is 0"),
    "cb column stride 0": (dict(cb=_ffi.view(CB_AT, (HC * WC, 1, WC, 0))), "column stride is 0"),
    "cr image stride 0 with two images": (dict(cr=_ffi.view(CR_AT, (0, 1, WC, 1))), "image stride is 0"),
    "y over cb": (dict(y=_ffi.view(FAKE + 2, YS)), "Y plane and a chroma plane overlap"),
    "cr is cb": (dict(cr=_ffi.view(CB_AT, CS)), "Cb and Cr planes overlap"),
    "cr one element behind a planar cb": (dict(cr=_ffi.view(CB_AT + 2, CS)), "Cb and Cr planes overlap"),
    "cr one row behind cb": (dict(cr=_ffi.view(CB_AT + 2 * WC, CS)), "Cb and Cr planes overlap"),
    "444: cr half a plane behind cb": (dict(sub=2, cr=_ffi.view(layout(10, 2)[5] + H * W, layout(10, 2)[4])), "Cb and Cr planes overlap"),
})


@pytest.mark.parametrize("name", sorted(TO_RGB_REFUSED))
def test_mz_ycbcr_to_rgb_refuses(name):
    kw, word = TO_RGB_REFUSED[name]
    code, msg = call("to_rgb", **kw)
    assert code == INVALID and word in msg, (name, code, msg)


@pytest.mark.parametrize("name", sorted(TO_YCBCR_REFUSED))
def test_mz_rgb_to_ycbcr_refuses(name):
    kw, word = TO_YCBCR_REFUSED[name]
    code, msg = call("to_ycbcr", **kw)
    assert code == INVALID and word in msg, (name, code, msg)


@pytest.mark.parametrize("direction", ["to_rgb", "to_ycbcr"])
@pytest.mark.parametrize("depth, align, sub", [(8, 0, 0), (8, 1, 2), (10, 1, 0), (10, 0, 1), (12, 1, 2), (16, 0, 0), (16, 1, 1)])
def test_dense_planes_of_every_format_pass_every_view_check(direction, depth, align, sub):
    code, msg = call(direction, depth=depth, align=align, sub=sub, siting=BAD_SITING)
    assert code == INVALID and "siting must be" in msg, (code, msg)


# frame buffers at FAKE, in ELEMENTS: H * W of Y, then the chroma of the frame
def chroma_case(depth, sub, cb_at, cr_at, strides, cr_strides=None, frames=True, byte_off=0):
    """Cb and Cr `cb_at`, `cr_at` ELEMENTS into the chroma part of frame buffers (Cr: plus `byte_off` bytes)"""
    es, hc, wc, _, _, _, _ = layout(depth, sub)
    frame = H * W + 2 * hc * wc
    y = _ffi.view(FAKE, (frame, 1, W, 1)) if frames else _ffi.view(FAR, YS)
    fix = lambda s: tuple(frame if v == "frame" else v for v in s)  # noqa: E731
    return dict(depth=depth, sub=sub, y=y, cb=_ffi.view(FAKE + es * (H * W + cb_at), fix(strides)),
                cr=_ffi.view(FAKE + es * (H * W + cr_at) + byte_off, fix(cr_strides or strides)))


def pairs(wc):
    return ("frame", 1, 2 * wc, 2)


def planar(wc):
    return ("frame", 1, wc, 1)


CHROMA_ACCEPTED = {
    "p010": dict(chroma_case(10, 0, 0, 1, pairs(W // 2)), align=1),
    "p016, cr first": dict(chroma_case(16, 0, 1, 0, pairs(W // 2)), align=1),
    "nv12 through the new entry": chroma_case(8, 0, 0, 1, pairs(W // 2)),
    "nv16, 12 bits": chroma_case(12, 1, 0, 1, pairs(W // 2)),
    "nv24": chroma_case(8, 2, 0, 1, pairs(W)),
    "yuv420p10le": chroma_case(10, 0, 0, (H // 2) * (W // 2), planar(W // 2)),
    "yuv422p10le, cr first": chroma_case(10, 1, H * (W // 2), 0, planar(W // 2)),
    "yuv444p16le": chroma_case(16, 2, 0, H * W, planar(W)),
    "column stride 4 elements, three elements apart": chroma_case(10, 0, 0, 3, (4 * HC * WC, 1, 4 * WC, 4), frames=False),
    "column stride 4 elements, three elements behind": chroma_case(10, 0, 3, 0, (4 * HC * WC, 1, 4 * WC, 4), frames=False),
}
def far_y(*args, **kw):
    return chroma_case(*args, frames=False, **kw)


CHROMA_REFUSED = {
    "the same interleaved view twice": (far_y(10, 0, 0, 0, pairs(W // 2)), "Cb and Cr planes overlap"),
    "a whole pair apart": (far_y(10, 0, 0, 2, pairs(W // 2)), "Cb and Cr planes overlap"),
    "cr one BYTE behind a 16-bit cb": (far_y(10, 0, 0, 0, pairs(W // 2), byte_off=1), "aligned to 2 bytes"),
    "column stride 4, four elements apart": (far_y(12, 0, 0, 4, (4 * HC * WC, 1, 4 * WC, 4), ), "Cb and Cr planes overlap"),
    "interleaved bases, different row strides": (far_y(10, 0, 0, 1, pairs(W // 2), ("frame", 1, 2 * W, 2)), "Cb and Cr planes overlap"),
    "one element apart with column stride 1": (far_y(16, 0, 0, 1, planar(W // 2)), "Cb and Cr planes overlap"),
    "planar, half a plane apart": (far_y(10, 1, 0, H * (W // 2) // 2, planar(W // 2)), "Cb and Cr planes overlap"),
    "negative column stride -2, one element apart": (far_y(10, 0, W - 2, W - 1, ("frame", 1, W, -2)), "Cb and Cr planes overlap"),
}


@pytest.mark.parametrize("name", sorted(CHROMA_ACCEPTED))
def test_chroma_layouts_that_are_accepted_pass_every_view_check(name):
    code, msg = call("to_ycbcr", siting=BAD_SITING, **CHROMA_ACCEPTED[name])
    assert code == INVALID and "siting must be" in msg, (name, code, msg)


@pytest.mark.parametrize("name", sorted(CHROMA_REFUSED))
def test_chroma_views_that_alias_are_refused(name):
    kw, word = CHROMA_REFUSED[name]
    code, msg = call("to_ycbcr", **kw)
    assert code == INVALID and word in msg, (name, code, msg)


def test_planes_that_only_read_may_alias_each_other():
    same = _ffi.view(CB_AT, CS)
    code, msg = call("to_rgb", cb=same, cr=same, siting=BAD_SITING)
    assert code == INVALID and "siting must be" in msg, (code, msg)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
FRAME_LAYOUTS = list(itertools.product(("semiplanar", "planar"), ("uv", "vu"), SUBSAMPLINGS, (np.uint8, np.uint16)))


@pytest.mark.parametrize("layout_, order, sub, dtype", FRAME_LAYOUTS, ids=lambda v: getattr(v, "__name__", v))
def test_frame_planes_against_plain_indexing(layout_, order, sub, dtype):
    from ultrazoom_amd import frame_planes

    b, h, w = 2, 4, 6
    hc, wc = ycbcr_ref.chroma_hw(h, w, sub)
    n = h * w + 2 * hc * wc + 5  # five elements of slack behind each frame
    a = (np.arange(b * n, dtype=np.int64) * 7 % 251 + (300 if dtype == np.uint16 else 0)).astype(dtype).reshape(b, n)
    buf = torch.from_numpy(a)
    y, cb, cr = frame_planes(buf, h, w, layout=layout_, order=order, subsampling=sub)
    assert y.shape == (b, 1, h, w) and cb.shape == cr.shape == (b, 1, hc, wc) and y.dtype == cb.dtype == cr.dtype == buf.dtype
    chroma = a[:, h * w:h * w + 2 * hc * wc]
    first, second = (chroma[:, 0::2], chroma[:, 1::2]) if layout_ == "semiplanar" else (chroma[:, :hc * wc], chroma[:, hc * wc:])
    want_cb, want_cr = (first, second) if order == "uv" else (second, first)
    assert np.array_equal(y.numpy().reshape(b, -1), a[:, :h * w])
    assert np.array_equal(cb.numpy().reshape(b, -1), want_cb) and np.array_equal(cr.numpy().reshape(b, -1), want_cr)
    for t in (y, cb, cr):  # views: nothing is copied
        assert t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    if layout_ == "semiplanar":
        assert cb.stride(3) == cr.stride(3) == 2 and abs(cb.data_ptr() - cr.data_ptr()) == buf.element_size()


def test_frame_planes_refusals():
    from ultrazoom_amd import frame_planes

    buf = torch.zeros(2, 100, dtype=torch.uint8)
    for kw in (dict(H=3, W=4), dict(H=4, W=5), dict(H=4, W=5, subsampling="422"), dict(H=8, W=12), dict(H=0, W=4), dict(H=4, W=4, layout="packed"),
               dict(H=4, W=4, order="yuv"), dict(H=4, W=4, subsampling="411"), dict(H=6, W=8, subsampling="444")):
        with pytest.raises(ValueError):
            frame_planes(buf, **kw)
    for bad in (torch.zeros(2, 100), torch.zeros(2, 100, dtype=torch.int16), torch.zeros(100, dtype=torch.uint8), torch.zeros(2, 10, 10, dtype=torch.uint8),
                torch.zeros(2, 200, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            frame_planes(bad, 4, 4)
    assert frame_planes(buf, 3, 4, subsampling="422")[1].shape == (2, 1, 3, 2)  # an odd H is halved by 4:2:0 only
    assert frame_planes(buf, 3, 5, subsampling="444")[1].shape == (2, 1, 3, 5)
    assert frame_planes(buf, 8, 8)[0].shape == (2, 1, 8, 8)  # 96 of 100 elements


def u16(*shape):
    return torch.from_numpy(np.zeros(shape, dtype=np.uint16))


def test_python_refusals_come_from_shapes_and_dtypes_alone():
    """on CPU tensors: a ValueError for every wrong shape, dtype, depth or name, before the device is looked at; right arguments reach
    the 'no CPU path' error"""
    from ultrazoom_amd import rgb_to_ycbcr, ycbcr_to_rgb, yuv420_to_rgb

    y8, c8 = torch.zeros(2, 1, 5, 7, dtype=torch.uint8), torch.zeros(2, 1, 3, 4, dtype=torch.uint8)
    y, c, c422, c444 = u16(2, 1, 5, 7), u16(2, 1, 3, 4), u16(2, 1, 5, 4), u16(2, 1, 5, 7)
    with pytest.raises(ValueError, match="depth"):
        ycbcr_to_rgb(y, c, c)  # uint16: the caller says which depth
    for kw in (dict(depth=8), dict(depth=9), dict(depth=11), dict(depth="10"), dict(depth=10, align="msb"), dict(depth=10, subsampling="411"),
               dict(depth=10, subsampling="422"), dict(depth=10, subsampling="444"), dict(depth=10, matrix="bt2100"), dict(depth=10, range="tv"),
               dict(depth=10, siting="top"), dict(depth=10, dtype=torch.float64), dict(depth=10, out=torch.zeros(2, 3, 5, 8))):
        with pytest.raises(ValueError):
            ycbcr_to_rgb(y, c, c, **kw)
    for kw in (dict(depth=10), dict(depth=16), dict(depth=12, align="high")):
        with pytest.raises(ValueError):
            ycbcr_to_rgb(y8, c8, c8, **kw)  # a depth that does not fit uint8
    for args in ((y[:, 0], c, c), (y, c[..., :3], c), (y, c, c8), (y, c8, c), (y.to(torch.int32), c, c), (y[:0], c[:0], c[:0])):
        with pytest.raises(ValueError):
            ycbcr_to_rgb(*args, depth=10)
    with pytest.raises(ValueError):
        yuv420_to_rgb(y8, c8, c8, matrix="bt2020")  # the 4:2:0 entries keep their two matrices
    for args, kw in (((y, c, c), dict(depth=10)), ((y, c, c), dict(depth=16, align="high", matrix="bt2020")), ((y8, c8, c8), {}), ((y8, c8, c8), dict(depth=8)),
                     ((y, c422, c422), dict(depth=12, subsampling="422")), ((y, c444, c444), dict(depth=10, subsampling="444", siting="center"))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ycbcr_to_rgb(*args, **kw)
    x = torch.zeros(2, 3, 5, 7)
    for kw in (dict(depth=9), dict(depth=None), dict(align="top"), dict(subsampling=420), dict(matrix=2), dict(range="limited "), dict(siting=None),
               dict(out=(y8, c8)), dict(depth=10, out=(y8, c8, c8)), dict(depth=8, out=(y, c, c)), dict(depth=10, out=(y, c, c422)),
               dict(depth=10, subsampling="422", out=(y, c, c)), dict(depth=10, out=(y[..., :6], c, c))):
        with pytest.raises(ValueError):
            rgb_to_ycbcr(x, **kw)
    for bad in (x[:, :2], x[0], x.double(), x[:, :, :0]):
        with pytest.raises(ValueError):
            rgb_to_ycbcr(bad, depth=10)
    for kw in ({}, dict(depth=10, align="high"), dict(depth=10, out=(y, c, c)), dict(depth=16, subsampling="444", matrix="bt2020", out=(y, c444, c444)),
               dict(out=(y8, c8, c8))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            rgb_to_ycbcr(x, **kw)
