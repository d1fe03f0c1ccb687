"""mz_ycbcr_to_rgb and mz_rgb_to_ycbcr on the GPU against the exact-arithmetic reference (tests/ycbcr_ref.py), bit for bit: every shape of
yuv_ref.SHAPES, the four RGB element types, every depth, alignment and subsampling with matrix, range, siting and clamp cycled over the
cases; depth 8 and 4:2:0 against the 4:2:0 entries; the container layouts of frame_planes, aligned and one element off; strided RGB
views and BGR; the round trip; MewZoom.upscale_ycbcr against the three calls it is made of."""

import itertools

import numpy as np
import pytest
import torch

import color_ref
import ycbcr_ref
import yuv_ref
from color_ref import DTYPES, same_bits
from model_util import lower_built
from ultrazoom_amd import frame_planes, rgb_to_ycbcr, rgb_to_yuv420, ycbcr_to_rgb, yuv420_to_rgb
from ycbcr_ref import FORMATS, PARAMS, SHAPES, put, same_words, tensor, words

pytestmark = pytest.mark.gpu

IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731
DT_LIST = sorted(DTYPES)


def case_params(fi, shape, dt):
    """one of PARAMS for format fi of a test case: the list is walked over the formats, from a start the shape and the dtype move"""
    return PARAMS[(fi + 5 * SHAPES.index(shape) + 7 * DT_LIST.index(dt)) % len(PARAMS)]


def planes_equal(got, want, what):
    for name, g, w in zip("y cb cr".split(), got, want):
        assert same_words(g, w), (what, name, g.dtype, tuple(g.shape), w.dtype, w.shape)


@pytest.mark.parametrize("dt", DT_LIST)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ycbcr_to_rgb_has_the_bits_of_the_reference(shape, dt):
    H, W = shape
    seen = set()
    for fi, (depth, align, sub) in enumerate(FORMATS):
        matrix, range_, siting, clamp = case_params(fi, shape, dt)
        seen.add((matrix, range_, siting, clamp))
        clamp = 1 if dt == "u8" else clamp
        planes = [tensor(p, "cuda") for p in ycbcr_ref.planes(3, H, W, depth, sub)]
        want = color_ref.store(ycbcr_ref.rgb_f64(3, H, W, depth, align, sub, matrix, range_, siting), dt, clamp)
        for B in (1, 3):
            got = ycbcr_to_rgb(*[t[:B] for t in planes], depth=depth, align=align, subsampling=sub, dtype=DTYPES[dt], matrix=matrix, range=range_,
                               siting=siting, clamp=bool(clamp))
            assert got.dtype == DTYPES[dt] and same_bits(got, want[:B]), (depth, align, sub, matrix, range_, siting, clamp, B)
    assert len(seen) == len(PARAMS)


@pytest.mark.parametrize("dt", DT_LIST)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rgb_to_ycbcr_has_the_bits_of_the_reference(shape, dt):
    H, W = shape
    x = color_ref.image(3, H, W, dt).cuda()
    for fi, (depth, align, sub) in enumerate(FORMATS):
        matrix, range_, siting, _ = case_params(fi, shape, dt)
        want = ycbcr_ref.ycbcr_of_image(3, H, W, dt, depth, align, sub, matrix, range_, siting)
        for B in (1, 3):
            got = rgb_to_ycbcr(x[:B], depth=depth, align=align, subsampling=sub, matrix=matrix, range=range_, siting=siting)
            planes_equal(got, [w[:B] for w in want], (depth, align, sub, matrix, range_, siting, B))
            if align == "high" and depth in (10, 12):
                assert all(int((words(g) & (2 ** (16 - depth) - 1)).max()) == 0 for g in got)  # the low bits are zero


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_depth_8_and_420_have_the_bits_of_the_420_entries(shape):
    for dt in DT_LIST:
        depth_8_and_420(shape, dt)


def depth_8_and_420(shape, dt):
    H, W = shape
    planes = [t.cuda() for t in yuv_ref.planes(3, H, W)]
    x = color_ref.image(3, H, W, dt).cuda()
    for matrix, range_, siting in itertools.product(sorted(yuv_ref.MATRIX_CODE), sorted(yuv_ref.RANGE_CODE), yuv_ref.SITINGS):
        kw = dict(matrix=matrix, range=range_, siting=siting)
        for clamp in ((True,) if dt == "u8" else (False, True)):
            want = yuv420_to_rgb(*planes, dtype=DTYPES[dt], clamp=clamp, **kw)
            for align in ("low", "high"):
                assert same_bits(ycbcr_to_rgb(*planes, depth=8, align=align, dtype=DTYPES[dt], clamp=clamp, **kw), want.cpu()), (kw, clamp)
        want = rgb_to_yuv420(x, **kw)
        for g, w in zip(rgb_to_ycbcr(x, **kw), want):
            assert g.dtype == torch.uint8 and torch.equal(g, w), kw


# ---- views -------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = list(itertools.product(("semiplanar", "planar"), ("uv", "vu")))
VIEW_FORMATS = [(8, "low", "422"), (8, "low", "444"), (10, "high", "420"), (10, "low", "420"), (12, "low", "422"), (16, "high", "444")]
TWO_PARAMS = [("bt2020", "limited", "left"), ("bt601", "full", "center")]


def frame_buffer(B, H, W, depth, sub, misalign=0):
    """a [B, n] buffer of 0xA5 bytes, n the frame's element count rounded up to 16 elements; misalign: its first element lies that many
    elements behind a 16-byte aligned address"""
    hc, wc = ycbcr_ref.chroma_hw(H, W, sub)
    n = -(-(H * W + 2 * hc * wc) // 16) * 16
    flat = tensor(np.full(B * n + misalign, 0xA5A5 if depth > 8 else 0xA5, dtype=ycbcr_ref.sample_dtype(depth)), "cuda")
    return flat[misalign:].view(B, n)


@pytest.mark.parametrize("fmt", VIEW_FORMATS, ids=lambda f: f"{f[0]}{f[1]}{f[2]}")
@pytest.mark.parametrize("shape, misalign", [((4, 32), 0), ((6, 48), 0), ((4, 32), 1)], ids=lambda v: IDS(v) if isinstance(v, tuple) else f"off{v}")
def test_container_layouts_are_views_of_the_same_planes(shape, misalign, fmt):
    """the three planes inside a semi-planar or planar frame buffer of either order, read and written in place: the bits of dense planes.
    Aligned buffers with 32- and 48-column rows take the 16-byte (pairs; 16-bit planes) and 8-byte (8-bit planes) accesses; a buffer that
    starts one element off takes the element path"""
    for layout, order in LAYOUTS:
        container_layout(shape, misalign, fmt, layout, order)


def container_layout(shape, misalign, fmt, layout, order):
    (H, W), B = shape, 2
    depth, align, sub = fmt
    dense = ycbcr_ref.planes(B, H, W, depth, sub)
    src = frame_buffer(B, H, W, depth, sub, misalign)
    assert src.data_ptr() % 16 == misalign * src.element_size()
    cut = dict(layout=layout, order=order, subsampling=sub)
    for v, d in zip(frame_planes(src, H, W, **cut), dense):
        put(v, d)
    for (matrix, range_, siting), dt in itertools.product(TWO_PARAMS, DT_LIST):
        kw = dict(depth=depth, align=align, subsampling=sub, matrix=matrix, range=range_, siting=siting)
        want = color_ref.store(ycbcr_ref.rgb_f64(B, H, W, depth, align, sub, matrix, range_, siting), dt, 1)
        assert same_bits(ycbcr_to_rgb(*frame_planes(src, H, W, **cut), dtype=DTYPES[dt], **kw), want), (dt, matrix)
        dst = frame_buffer(B, H, W, depth, sub, misalign)
        views = frame_planes(dst, H, W, **cut)
        got = rgb_to_ycbcr(color_ref.image(B, H, W, dt).cuda(), out=views, **kw)
        assert all(g is v for g, v in zip(got, views))
        planes_equal(frame_planes(dst, H, W, **cut), ycbcr_ref.ycbcr_of_image(B, H, W, dt, depth, align, sub, matrix, range_, siting), (dt, matrix))
        hc, wc = ycbcr_ref.chroma_hw(H, W, sub)
        slack = words(dst[:, H * W + 2 * hc * wc:])
        assert (slack == (0xA5A5 if depth > 8 else 0xA5)).all()  # the elements behind a frame keep what they held


def rgb_views(B, H, W, dtype):
    def new(*shape):
        return torch.empty(shape, dtype=dtype, device="cuda")

    return {
        "channels_last": new(B, H, W, 3).permute(0, 3, 1, 2),
        "crop": new(B, 3, H + 5, W + 7)[:, :, 2:2 + H, 3:3 + W],
        "every second image": new(2 * B, 3, H, W)[::2],
    }


@pytest.mark.parametrize("dt", DT_LIST)
@pytest.mark.parametrize("shape", [(3, 3), (4, 32), (5, 33), (7, 129)], ids=IDS)
def test_strided_rgb_views_on_both_sides(shape, dt):
    (H, W), B = shape, 2
    x = color_ref.image(B, H, W, dt)
    for (depth, align, sub), (matrix, range_, siting) in zip([(10, "high", "420"), (12, "low", "422"), (16, "low", "444"), (8, "low", "444")], TWO_PARAMS * 2):
        kw = dict(depth=depth, align=align, subsampling=sub, matrix=matrix, range=range_, siting=siting)
        planes = [tensor(p, "cuda") for p in ycbcr_ref.planes(B, H, W, depth, sub)]
        want_rgb = color_ref.store(ycbcr_ref.rgb_f64(B, H, W, depth, align, sub, matrix, range_, siting), dt, 0 if dt != "u8" else 1)
        want = ycbcr_ref.ycbcr_of_image(B, H, W, dt, depth, align, sub, matrix, range_, siting)
        for name, v in rgb_views(B, H, W, DTYPES[dt]).items():
            got = ycbcr_to_rgb(*planes, clamp=dt == "u8", out=v, **kw)
            assert got is v and same_bits(v.contiguous(), want_rgb), (name, kw)
            v.copy_(x)
            planes_equal(rgb_to_ycbcr(v, **kw), want, (name, kw))


@pytest.mark.parametrize("dt", DT_LIST)
def test_bgr_tensors_through_a_negative_channel_stride(dt):
    """the C entries take signed strides: a BGR tensor read and written as RGB, its red plane the base of the view"""
    from ultrazoom_amd import _ffi

    B, H, W = 2, 6, 40
    depth, align, sub, matrix, range_, siting = 10, "high", "420", "bt2020", "limited", "left"
    fmt, codes = _ffi.ycbcr_codes(depth, align, sub, matrix, range_, siting)
    stream = torch.cuda.current_stream().cuda_stream
    planes = [tensor(p, "cuda") for p in ycbcr_ref.planes(B, H, W, depth, sub)]
    bgr = torch.empty((B, 3, H, W), dtype=DTYPES[dt], device="cuda")
    red = (bgr[:, 2:].data_ptr(), (3 * H * W, -H * W, W, 1))
    _ffi.ycbcr_to_rgb(*[_ffi.pair(t) for t in planes], *fmt, red, color_ref.ELEM[dt], B, H, W, *codes, 1, stream)
    assert same_bits(bgr.flip(1), color_ref.store(ycbcr_ref.rgb_f64(B, H, W, depth, align, sub, matrix, range_, siting), dt, 1))
    bgr.copy_(color_ref.image(B, H, W, dt).flip(1))
    got = [torch.empty_like(t) for t in planes]
    _ffi.rgb_to_ycbcr(red, color_ref.ELEM[dt], *[_ffi.pair(t) for t in got], *fmt, B, H, W, *codes, stream)
    planes_equal(got, ycbcr_ref.ycbcr_of_image(B, H, W, dt, depth, align, sub, matrix, range_, siting), dt)


# ---- round trip ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", ycbcr_ref.DEPTHS)
@pytest.mark.parametrize("matrix", sorted(ycbcr_ref.MATRIX_CODE))
def test_round_trip_through_float32_returns_the_planes(matrix, depth):
    for (H, W), sub, (range_, siting, align) in zip([(1, 1), (2, 2), (3, 5), (17, 33), (64, 130), (5, 18)], ycbcr_ref.SUBSAMPLINGS * 2,
                                                    [("limited", "left", "low"), ("full", "center", "high"), ("full", "left", "high")] * 2):
        planes = ycbcr_ref.grey_chroma_frames(2, H, W, depth, align, sub)
        kw = dict(depth=depth, align=align, subsampling=sub, matrix=matrix, range=range_, siting=siting)
        rgb = ycbcr_to_rgb(*[tensor(p, "cuda") for p in planes], dtype=torch.float32, clamp=False, **kw)
        planes_equal(rgb_to_ycbcr(rgb, **kw), planes, (H, W, kw))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def test_upscale_ycbcr_is_the_three_public_calls():
    model = lower_built("g1", torch.bfloat16)  # 2X
    B, H, W, r = 2, 16, 24, 2
    for (depth, align, sub, layout), (matrix, range_, siting) in zip([(10, "high", "420", "semiplanar"), (8, "low", "444", "planar"), (12, "low", "422", "planar")],
                                                                      TWO_PARAMS + TWO_PARAMS[:1]):
        kw = dict(depth=depth, align=align, subsampling=sub, matrix=matrix, range=range_, siting=siting)
        dense = [tensor(p, "cuda") for p in ycbcr_ref.planes(B, H, W, depth, sub)]
        got = model.upscale_ycbcr(*dense, **kw)
        rgb = ycbcr_to_rgb(*dense, dtype=torch.bfloat16, clamp=True, **kw)
        want = [words(t) for t in rgb_to_ycbcr(model.upscale(rgb), **kw)]
        hc, wc = ycbcr_ref.chroma_hw(r * H, r * W, sub)
        assert tuple(got[0].shape) == (B, 1, r * H, r * W) and tuple(got[1].shape) == tuple(got[2].shape) == (B, 1, hc, wc)
        assert got[0].dtype == dense[0].dtype
        planes_equal(got, want, "dense")
        assert len(set(want[0].flatten().tolist())) > 16  # a picture, not a constant
        src = frame_planes(frame_buffer(B, H, W, depth, sub), H, W, layout=layout, subsampling=sub)
        for v, d in zip(src, dense):
            put(v, d)
        dst = frame_buffer(B, r * H, r * W, depth, sub)
        views = frame_planes(dst, r * H, r * W, layout=layout, subsampling=sub)
        ret = model.upscale_ycbcr(*src, out=views, **kw)
        assert all(a is b for a, b in zip(ret, views))
        planes_equal(frame_planes(dst, r * H, r * W, layout=layout, subsampling=sub), want, layout + " out")
