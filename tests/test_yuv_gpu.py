"""mz_yuv420_to_rgb and mz_rgb_to_yuv420 on the GPU against the exact-arithmetic reference (tests/yuv_ref.py), bit for bit: every shape
of yuv_ref.SHAPES (odd sides, edge clamps, runs below, at and above 16 bytes, several workgroups), one and three images, both matrices,
ranges and sitings, the four RGB element types, the clamp on and off; the four container layouts and strided RGB views on both sides;
the round trip; MewZoom.upscale_yuv420 against the three calls it is made of."""

import itertools

import pytest
import torch

import color_ref
import yuv_ref
from color_ref import DTYPES, same_bits
from model_util import lower_built
from ultrazoom_amd import i420_planes, nv12_planes, rgb_to_yuv420, yuv420_to_rgb
from yuv_ref import MATRIX_CODE, RANGE_CODE, SHAPES, SITINGS

pytestmark = pytest.mark.gpu

PARAMS = list(itertools.product(sorted(MATRIX_CODE), sorted(RANGE_CODE), SITINGS))
TWO_PARAMS = [("bt709", "limited", "left"), ("bt601", "full", "center")]
IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def planes_equal(got, want, what):
    for name, g, w in zip("y cb cr".split(), got, want):
        assert g.dtype == torch.uint8 and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, g.shape, w.shape)
        assert torch.equal(g.cpu(), w), (what, name, int((g.cpu() != w).sum()))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_yuv420_to_rgb_has_the_bits_of_the_reference(shape, dt):
    H, W = shape
    planes = [t.cuda() for t in yuv_ref.planes(3, H, W)]
    for matrix, range_, siting in PARAMS:
        f64 = yuv_ref.rgb_f64(3, H, W, matrix, range_, siting)
        for clamp in ((1,) if dt == "u8" else (0, 1)):
            want = color_ref.store(f64, dt, clamp)
            for B in (1, 3):
                got = yuv420_to_rgb(*[t[:B] for t in planes], dtype=DTYPES[dt], matrix=matrix, range=range_, siting=siting, clamp=bool(clamp))
                assert got.dtype == DTYPES[dt] and same_bits(got, want[:B]), (matrix, range_, siting, clamp, B)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rgb_to_yuv420_has_the_bits_of_the_reference(shape, dt):
    H, W = shape
    x = color_ref.image(3, H, W, dt).cuda()
    for matrix, range_, siting in PARAMS:
        want = yuv_ref.yuv_of_image(3, H, W, dt, matrix, range_, siting)
        for B in (1, 3):
            got = rgb_to_yuv420(x[:B], matrix=matrix, range=range_, siting=siting)
            planes_equal(got, [w[:B] for w in want], (matrix, range_, siting, B))


# ---- views -------------------------------------------------------------------------------------------------------------------------------
CONTAINERS = {"nv12": (nv12_planes, "uv"), "nv21": (nv12_planes, "vu"), "i420": (i420_planes, "uv"), "yv12": (i420_planes, "vu")}


def frame_buffer(B, H, W, misalign=0):
    """a [B, H * 3 / 2, W] uint8 buffer of 0xA5 bytes; misalign: its first byte lies that many bytes behind an aligned address"""
    n = B * (H * 3 // 2) * W
    return torch.full((n + misalign,), 0xA5, dtype=torch.uint8, device="cuda")[misalign:].view(B, H * 3 // 2, W)


@pytest.mark.parametrize("layout", sorted(CONTAINERS))
@pytest.mark.parametrize("shape, misalign", [((4, 32), 0), ((6, 48), 0), ((18, 258), 0), ((4, 32), 1), ((6, 48), 8)],
                         ids=lambda v: IDS(v) if isinstance(v, tuple) else f"off{v}")
def test_container_layouts_are_views_of_the_same_planes(shape, misalign, layout):
    """the three planes inside an NV12 / NV21 / I420 / YV12 frame buffer, read and written in place: the bits of dense planes.  32- and
    48-byte rows at an aligned address take the 16-byte (NV12: pair) and 8-byte (I420) accesses; 258-byte rows and buffers that start
    1 or 8 bytes off take the element path (8 bytes off: I420's chroma rows stay 8-byte aligned, Y's are not 16-byte aligned)"""
    (H, W), B = shape, 2
    cut, order = CONTAINERS[layout]
    dense = yuv_ref.planes(B, H, W)
    src = frame_buffer(B, H, W, misalign)
    assert src.data_ptr() % 16 == misalign
    for v, d in zip(cut(src, order=order), dense):
        v.copy_(d)
    for (matrix, range_, siting), dt in itertools.product(TWO_PARAMS, sorted(DTYPES)):
        kw = dict(matrix=matrix, range=range_, siting=siting)
        want = color_ref.store(yuv_ref.rgb_f64(B, H, W, matrix, range_, siting), dt, 1)
        assert same_bits(yuv420_to_rgb(*cut(src, order=order), dtype=DTYPES[dt], **kw), want), (dt, matrix)
        dst = frame_buffer(B, H, W, misalign)
        views = cut(dst, order=order)
        got = rgb_to_yuv420(color_ref.image(B, H, W, dt).cuda(), out=views, **kw)
        assert all(g is v for g, v in zip(got, views))
        planes_equal(cut(dst, order=order), yuv_ref.yuv_of_image(B, H, W, dt, matrix, range_, siting), (dt, matrix))


def rgb_views(B, H, W, dtype):
    """name -> an uninitialised [B, 3, H, W] view (BGR, a negative channel stride, is no torch view: the test below)"""
    def new(*shape):
        return torch.empty(shape, dtype=dtype, device="cuda")

    return {
        "channels_last": new(B, H, W, 3).permute(0, 3, 1, 2),
        "crop": new(B, 3, H + 5, W + 7)[:, :, 2:2 + H, 3:3 + W],
        "every second image": new(2 * B, 3, H, W)[::2],
    }


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(3, 3), (4, 32), (5, 33), (7, 129)], ids=IDS)
def test_strided_rgb_views_on_both_sides(shape, dt):
    (H, W), B = shape, 2
    planes = [t.cuda() for t in yuv_ref.planes(B, H, W)]
    x = color_ref.image(B, H, W, dt)
    for matrix, range_, siting in TWO_PARAMS:
        want_rgb = color_ref.store(yuv_ref.rgb_f64(B, H, W, matrix, range_, siting), dt, 0 if dt != "u8" else 1)
        want_yuv = yuv_ref.yuv_of_image(B, H, W, dt, matrix, range_, siting)
        for name, v in rgb_views(B, H, W, DTYPES[dt]).items():
            got = yuv420_to_rgb(*planes, matrix=matrix, range=range_, siting=siting, clamp=dt == "u8", out=v)
            assert got is v and same_bits(v.contiguous(), want_rgb), (name, matrix)
            v.copy_(x)
            planes_equal(rgb_to_yuv420(v, matrix=matrix, range=range_, siting=siting), want_yuv, (name, matrix))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_bgr_tensors_through_a_negative_channel_stride(dt):
    """the C entries take signed strides: a BGR tensor read and written as RGB, its red plane the base of the view"""
    from ultrazoom_amd import _ffi

    B, H, W = 2, 6, 40
    matrix, range_, siting = "bt709", "limited", "left"
    codes = (MATRIX_CODE[matrix], RANGE_CODE[range_], yuv_ref.SITING_CODE[siting])
    stream = torch.cuda.current_stream().cuda_stream
    planes = [t.cuda() for t in yuv_ref.planes(B, H, W)]
    bgr = torch.empty((B, 3, H, W), dtype=DTYPES[dt], device="cuda")
    red = (bgr[:, 2:].data_ptr(), (3 * H * W, -H * W, W, 1))
    _ffi.yuv420_to_rgb(*[_ffi.pair(t) for t in planes], red, color_ref.ELEM[dt], B, H, W, *codes, 1, stream)
    assert same_bits(bgr.flip(1), color_ref.store(yuv_ref.rgb_f64(B, H, W, matrix, range_, siting), dt, 1))
    bgr.copy_(color_ref.image(B, H, W, dt).flip(1))
    got = [torch.empty_like(t) for t in planes]
    _ffi.rgb_to_yuv420(red, color_ref.ELEM[dt], *[_ffi.pair(t) for t in got], B, H, W, *codes, stream)
    planes_equal(got, yuv_ref.yuv_of_image(B, H, W, dt, matrix, range_, siting), dt)


# ---- round trip ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix, range_, siting", PARAMS, ids=lambda v: v)
def test_round_trip_through_float32_returns_the_planes(matrix, range_, siting):
    for H, W in [(1, 1), (2, 2), (3, 5), (17, 33), (64, 130)]:
        planes = yuv_ref.grey_chroma_frames(2, H, W)
        rgb = yuv420_to_rgb(*[t.cuda() for t in planes], dtype=torch.float32, matrix=matrix, range=range_, siting=siting, clamp=False)
        planes_equal(rgb_to_yuv420(rgb, matrix=matrix, range=range_, siting=siting), planes, (H, W))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def test_upscale_yuv420_is_the_three_public_calls():
    model = lower_built("g1", torch.bfloat16)  # 2X
    B, H, W, r = 2, 16, 24, 2
    dense = [t.cuda() for t in yuv_ref.planes(B, H, W)]
    for matrix, range_, siting in TWO_PARAMS:
        kw = dict(matrix=matrix, range=range_, siting=siting)
        got = model.upscale_yuv420(*dense, **kw)
        rgb = yuv420_to_rgb(*dense, dtype=torch.bfloat16, clamp=True, **kw)
        want = [t.cpu() for t in rgb_to_yuv420(model.upscale(rgb), **kw)]
        assert tuple(got[0].shape) == (B, 1, r * H, r * W) and tuple(got[1].shape) == tuple(got[2].shape) == (B, 1, r * H // 2, r * W // 2)
        planes_equal(got, want, "dense")
        assert len(set(want[0].flatten().tolist())) > 16  # a picture, not a constant
        for layout, (cut, order) in sorted(CONTAINERS.items()):
            src = cut(frame_buffer(B, H, W), order=order)
            for v, d in zip(src, dense):
                v.copy_(d)
            planes_equal(model.upscale_yuv420(*src, **kw), want, layout)
            dst = frame_buffer(B, r * H, r * W)
            views = cut(dst, order=order)
            ret = model.upscale_yuv420(*src, out=views, **kw)
            assert all(a is b for a, b in zip(ret, views))
            planes_equal(cut(dst, order=order), want, layout + " out")
