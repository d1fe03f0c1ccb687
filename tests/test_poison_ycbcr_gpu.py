"""mz_ycbcr_to_rgb and mz_rgb_to_ycbcr in poisoned surroundings (tests/poison_util.py), in the manner of tests/test_poison_yuv_gpu.py: frame
buffers of every layout of frame_planes between 0xFF (NaN) or 0x00 guards as inputs and between pattern guards as outputs, an odd-sized
frame of dense planes, and planes with padding between their rows.  The results have the bits of the reference -- so no poisoned byte
next to an input has reached an output -- and no guard, no padding and no input has changed.  A test of loads and stores staying inside
their tensors: every run here is an ordinary, valid call."""

import itertools

import numpy as np
import pytest
import torch

import color_ref
import ycbcr_ref
from color_ref import DTYPES, ELEM
from poison_util import Arena
from ultrazoom_amd import _ffi, frame_planes
from ycbcr_ref import same_words, words

pytestmark = pytest.mark.gpu

B = 2
LAYOUTS = list(itertools.product(("semiplanar", "planar"), ("uv", "vu"), ycbcr_ref.SUBSAMPLINGS))
FORMATS = [(8, "low"), (10, "high"), (12, "low")]
CASES = [("bt2020", "limited", "left"), ("bt601", "full", "center")]
SHAPES = [(4, 32), (6, 34), (2, 2)]  # whole runs; a ragged run of two columns behind two whole ones; one chroma sample


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def frame_bytes(planes, layout, order, sub):
    """the frames of dense planes (numpy words) as a [B, n] numpy array of words, as frame_planes reads them"""
    y, cb, cr = planes
    first, second = (cb, cr) if order == "uv" else (cr, cb)
    b = y.shape[0]
    chroma = np.stack([first, second], axis=-1) if layout == "semiplanar" else np.stack([first, second], axis=1)
    return np.concatenate([y.reshape(b, -1), chroma.reshape(b, -1)], axis=1)


def as_words(buf8, depth):
    """a [B, bytes] uint8 arena tensor as the [B, n] buffer of its samples"""
    return buf8.view(torch.uint16) if depth > 8 else buf8


def to_rgb_between_guards(layout, order, sub, depth, align, guard):
    fmt_codes = {}
    for (H, W), case, dt in zip(SHAPES * 2, CASES * 3, sorted(DTYPES) + ["bf16", "f32"]):
        fmt, codes = fmt_codes.setdefault(case, _ffi.ycbcr_codes(depth, align, sub, *case))
        planes = ycbcr_ref.planes(B, H, W, depth, sub)
        want = color_ref.store(ycbcr_ref.rgb_f64(B, H, W, depth, align, sub, *case), dt, 1)
        arena = Arena("cuda")
        frames = frame_bytes(planes, layout, order, sub)
        buf = as_words(arena.input(torch.from_numpy(frames.view(np.uint8)).cuda(), name="frames", fill=guard), depth)
        out = arena.output((B, 3, H, W), DTYPES[dt], fill=3, name="out")
        y, cb, cr = frame_planes(buf, H, W, layout=layout, order=order, subsampling=sub)
        _ffi.ycbcr_to_rgb(_ffi.pair(y), _ffi.pair(cb), _ffi.pair(cr), *fmt, _ffi.pair(out), ELEM[dt], B, H, W, *codes, 1, stream())
        arena.check()
        assert color_ref.same_bits(out, want), (H, W, case, dt)


def to_ycbcr_between_guards(layout, order, sub, depth, align, guard):
    es = 2 if depth > 8 else 1
    for (H, W), case, dt in zip(SHAPES * 2, CASES * 3, sorted(DTYPES) + ["bf16", "f32"]):
        fmt, codes = _ffi.ycbcr_codes(depth, align, sub, *case)
        want = ycbcr_ref.ycbcr_of_image(B, H, W, dt, depth, align, sub, *case)
        hc, wc = ycbcr_ref.chroma_hw(H, W, sub)
        arena = Arena("cuda")
        xa = arena.input(color_ref.image(B, H, W, dt).cuda(), name="x", fill=guard)
        buf = as_words(arena.output((B, (H * W + 2 * hc * wc) * es), torch.uint8, fill=3, name="frames"), depth)
        views = frame_planes(buf, H, W, layout=layout, order=order, subsampling=sub)
        _ffi.rgb_to_ycbcr(_ffi.pair(xa), ELEM[dt], *[_ffi.pair(v) for v in views], *fmt, B, H, W, *codes, stream())
        arena.check()
        assert same_words(buf, frame_bytes(want, layout, order, sub)), (H, W, case, dt)


@pytest.mark.parametrize("layout, order, sub", LAYOUTS, ids=lambda v: v)
def test_ycbcr_to_rgb_touches_its_frame_buffer_only(layout, order, sub):
    """every format of FORMATS between 0xFF (NaN) and between 0x00 guards"""
    for (depth, align), guard in itertools.product(FORMATS, (0xFF, 0x00)):
        to_rgb_between_guards(layout, order, sub, depth, align, guard)


@pytest.mark.parametrize("layout, order, sub", LAYOUTS, ids=lambda v: v)
def test_rgb_to_ycbcr_touches_its_frame_buffer_only(layout, order, sub):
    for (depth, align), guard in itertools.product(FORMATS, (0xFF, 0x00)):
        to_ycbcr_between_guards(layout, order, sub, depth, align, guard)


def padded(a, pad, fill):
    """[B,1,h,w] words -> [B,1,h,w + pad] with `fill` in the padding columns"""
    wide = np.full(a.shape[:-1] + (a.shape[-1] + pad,), fill, dtype=a.dtype)
    wide[..., : a.shape[-1]] = a
    return wide


@pytest.mark.parametrize("depth, align, sub", [(10, "high", "420"), (16, "low", "422"), (12, "high", "444"), (8, "low", "422"), (8, "high", "444")], ids=lambda v: v)
@pytest.mark.parametrize("shape, pad", [((5, 33), 0), ((3, 3), 0), ((4, 32), 8), ((7, 129), 3)], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"pad{v}")
def test_odd_frames_and_padded_rows_touch_their_elements_only(shape, pad, depth, align, sub):
    """dense planes of odd sizes; planes whose rows are pad elements apart (pad 8: the rows stay aligned, the wide accesses run next to the
    padding; pad 3: the element path): the padding holds all-ones words on the input side and keeps its fill on the output side; every RGB type"""
    for dt in sorted(DTYPES):
        odd_or_padded(shape, pad, depth, align, sub, dt)


def odd_or_padded(shape, pad, depth, align, sub, dt):
    H, W = shape
    case = CASES[(H + pad) % 2]
    fmt, codes = _ffi.ycbcr_codes(depth, align, sub, *case)
    es, ones = (2, 0xFFFF) if depth > 8 else (1, 0xFF)
    planes = ycbcr_ref.planes(B, H, W, depth, sub)
    # planes -> RGB
    arena = Arena("cuda")
    ins = [as_words(arena.input(torch.from_numpy(padded(p, pad, ones).view(np.uint8)).cuda(), name=n), depth)[..., : p.shape[-1]] for p, n in zip(planes, ("y", "cb", "cr"))]
    out = arena.output((B, 3, H, W + pad), DTYPES[dt], fill=3, name="out")
    _ffi.ycbcr_to_rgb(*[_ffi.pair(t) for t in ins], *fmt, _ffi.pair(out[..., :W]), ELEM[dt], B, H, W, *codes, 1, stream())
    arena.check()
    assert color_ref.same_bits(out[..., :W].contiguous(), color_ref.store(ycbcr_ref.rgb_f64(B, H, W, depth, align, sub, *case), dt, 1))
    assert pad == 0 or bool((out[..., W:] == 3).all())
    # RGB -> planes
    want = ycbcr_ref.ycbcr_of_image(B, H, W, dt, depth, align, sub, *case)
    arena = Arena("cuda")
    xa = arena.input(color_ref.image(B, H, W, dt).cuda(), name="x")
    outs = [as_words(arena.output(w.shape[:-1] + ((w.shape[-1] + pad) * es,), torch.uint8, fill=3, name=n), depth) for w, n in zip(want, ("y", "cb", "cr"))]
    _ffi.rgb_to_ycbcr(_ffi.pair(xa), ELEM[dt], *[_ffi.pair(o[..., : w.shape[-1]]) for o, w in zip(outs, want)], *fmt, B, H, W, *codes, stream())
    arena.check()
    for o, w in zip(outs, want):
        assert same_words(o[..., : w.shape[-1]], w)
        assert pad == 0 or bool((words(o[..., w.shape[-1]:]) == (0x0303 if depth > 8 else 3)).all())
