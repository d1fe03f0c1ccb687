"""Every image entry on far views (tests/far_util.py): a dense tensor placed inside one large allocation at strides whose offsets cross
2^31 and 2^32 -- an image stride of 2^31 + 40 elements, a channel stride past 2^32 bytes, a row pitch of 2^28 + 64 bytes, the first two
also negative.  Each entry runs once on dense tensors and once per variant on far views of the same data; the two results must have equal
BITS (the dense path is held to its float64 restatement by the entry's own module).  Around every row of a far view lie 64-byte guard
bands, which the call must leave unchanged; nothing else of an allocation is ever touched.

A variant names the kind of the far inputs, the kind of the far outputs and `misalign`: 0 keeps the base and every stride a multiple of
16 bytes, so that the 16-byte paths (store16, load16, the paired chroma accesses) run at the far offsets; an odd number of elements
breaks rows_aligned and the element paths run there.  The image kinds run two images, the others one; a pitch kind gives the far side
18 rows (rows 8.. start past 2^31 bytes, rows 16 and 17 past 2^32) -- the metrics entries keep their 43 rows, which VIF needs, and then take
one far input at a time (two would pass the 20e9-byte cap).  A one-channel plane stays dense under the channel kind.

Read views with strides of 0: every entry that admits them reads one stored plane, or one stored image, through a channel and an image
stride of 0 and must give the bits it gives for the expanded dense tensor.

mz_forward_view's input side: upscale_into of g1_2x_c16 on far inputs, through torch views (which cannot express the negative kinds)."""

import gc
import time
from collections import namedtuple

import pytest
import torch

import color_ref
import far_util as fu
import interp_util
import resize_util
import ycbcr_ref
import yuv_ref
from model_util import lower_built
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

DTYPES, ELEM = color_ref.DTYPES, color_ref.ELEM
KM = [("image", 0), ("image_neg", 1), ("channel", 1), ("pitch", 0), ("pitch_neg", 1), ("image", 1), ("image_neg", 0), ("channel", 0), ("pitch", 1),
      ("pitch_neg", 0)]
BOTH = [(("image", 0), ("image_neg", 0)), (("image_neg", 1), ("image", 1)), (("channel", 1), ("pitch", 0)), (("pitch", 0), ("channel", 0)),
        (("pitch_neg", 1), ("pitch", 1)), (("channel", 0), ("pitch_neg", 0)), (("pitch", 1), ("pitch_neg", 1)), (("pitch_neg", 0), ("channel", 1))]
# (kind and misalign of the far inputs or None, of the far outputs or None)
VARIANTS = [(km, None) for km in KM] + [(None, km) for km in KM] + BOTH


@pytest.fixture(autouse=True)
def release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def bits(t):
    """a tensor as integers of its element width: equality of these is equality of bit patterns"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def image(dt, B, H, W, seed=5):
    return color_ref.image(B, H, W, dt, seed=seed, special=False)


class Dense:
    """a dense device tensor with the interface of far_util.FarView"""

    def __init__(self, t):
        self.t = t
        self.pair = _ffi.pair(t)

    def read(self):
        return self.t

    def check_guards(self):
        pass


def fill_value(dtype):
    return 0x5A if dtype in (torch.uint8, torch.int16) else 7.0


def place(dense, km, write=True):
    """`dense` (a CPU tensor; an output: any tensor of its shape and dtype) as a far view of kind km = (kind, misalign), or dense where km
    is None or the kind does not apply to it (a one-channel plane under "channel")"""
    if km is None or (km[0] == "channel" and dense.shape[1] == 1):
        t = dense.cuda() if write else torch.full(dense.shape, fill_value(dense.dtype), dtype=dense.dtype, device="cuda")
        return Dense(t)
    v = fu.far_view(dense, km[0], km[1], device="cuda", write=write)
    return v if write else v.fill(fill_value(v.dtype))


# ins: dense CPU tensors; outs: (shape, dtype) of the views written; call(in pairs, out pairs) -> a tensor the call leaves elsewhere (the
# metrics' slots, the ensemble's accumulator) or None; one_far: only one input is far at a time (by the variant's index)
Run = namedtuple("Run", "ins outs call one_far", defaults=(False,))


def rows(base, *pitched):
    """`base` rows, or far_util.PITCH_H where a far side of this tensor is a pitch kind"""
    return fu.PITCH_H if any(pitched) else base


def e_luma(dt, B, pin, pout):
    H, W = rows(7, pin, pout), 129
    return Run([image(dt, B, H, W)], [((B, 1, H, W), DTYPES[dt])],
               lambda i, o: _ffi.luma(*i[0], *o[0], ELEM[dt], B, H, W, 0, 1, stream()))


def metrics_entry(luma):
    def make(dt, B, pin, pout):
        H, W, which = 43, 75, 7  # the tile-edge shape of tests/test_metrics_gpu.py that VIF admits (41 x 41 at least)
        need = (_ffi.metrics_luma_workspace_bytes if luma else _ffi.metrics_workspace_bytes)(B, H, W, which)

        def call(i, o):
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
            out = torch.zeros((B, _ffi.MZ_METRIC_SLOTS), dtype=torch.float64, device="cuda")
            if luma:
                _ffi.metrics_luma(*i[0], *i[1], ELEM[dt], B, H, W, which, 0, 1.0, 2.0, out.data_ptr(), ws.data_ptr(), need, stream())
            else:
                _ffi.metrics(*i[0], *i[1], ELEM[dt], B, H, W, which, 1.0, 2.0, out.data_ptr(), ws.data_ptr(), need, stream())
            return out

        clip = (lambda t: t) if dt == "u8" else (lambda t: t.float().clamp(0, 1).to(t.dtype))
        return Run([clip(image(dt, B, H, W, 5)), clip(image(dt, B, H, W, 6))], [], call, True)
    return make


YUV_CODES = _ffi.yuv_codes("bt709", "limited", "left")
HW = (18, 258)  # yuv_ref's "several workgroups" shape: 18 rows also serve the pitch kinds


def frame_of(planes, H):
    """Y above interleaved CbCr (NV12, P210): [B, 1, H + Hc, W] of the planes' dtype (W even)"""
    y, cb, cr = planes
    B, _, _, W = y.shape
    assert W % 2 == 0 and 2 * cb.shape[3] == W
    f = torch.zeros((B, 1, H + cb.shape[2], W), dtype=y.dtype)
    f[:, :, :H] = y
    f[:, :, H:, 0::2] = cb
    f[:, :, H:, 1::2] = cr
    return f


def frame_pairs(pair, H, es):
    """(y, cb, cr) pairs of a frame_of view: the chroma rows begin H rows behind, Cr one element behind Cb, column stride 2"""
    ptr, st = pair
    cb = ptr + H * st[2] * es
    return (ptr, st), (cb, (st[0], st[1], st[2], 2)), (cb + es, (st[0], st[1], st[2], 2))


def e_yuv_to_rgb(nv12):
    def make(dt, B, pin, pout):
        H, W = HW
        planes = yuv_ref.planes(B, H, W)

        def call(i, o):
            y, cb, cr = frame_pairs(i[0], H, 1) if nv12 else i
            _ffi.yuv420_to_rgb(y, cb, cr, o[0], ELEM[dt], B, H, W, *YUV_CODES, 1, stream())

        return Run([frame_of(planes, H)] if nv12 else list(planes), [((B, 3, H, W), DTYPES[dt])], call)
    return make


def e_rgb_to_yuv(nv12):
    def make(dt, B, pin, pout):
        H, W = HW
        Hc, Wc = yuv_ref.chroma_hw(H, W)

        def call(i, o):
            y, cb, cr = frame_pairs(o[0], H, 1) if nv12 else o
            _ffi.rgb_to_yuv420(i[0], ELEM[dt], y, cb, cr, B, H, W, *YUV_CODES, stream())

        outs = [((B, 1, H + Hc, W), torch.uint8)] if nv12 else [((B, 1, H, W), torch.uint8)] + [((B, 1, Hc, Wc), torch.uint8)] * 2
        return Run([image(dt, B, H, W)], outs, call)
    return make


def ycbcr_format(p210):
    return (10, "high", "422") if p210 else (8, "low", "420")


def e_ycbcr_to_rgb(p210):
    def make(dt, B, pin, pout):
        H, W = HW
        depth, align, sub = ycbcr_format(p210)
        fmt, codes = _ffi.ycbcr_codes(depth, align, sub, "bt2020", "limited", "center")
        planes = [ycbcr_ref.tensor(a) for a in ycbcr_ref.planes(B, H, W, depth, sub)]
        planes = [t.view(torch.int16) if t.dtype == torch.uint16 else t for t in planes]

        def call(i, o):
            y, cb, cr = frame_pairs(i[0], H, 2) if p210 else i
            _ffi.ycbcr_to_rgb(y, cb, cr, *fmt, o[0], ELEM[dt], B, H, W, *codes, 1, stream())

        return Run([frame_of(planes, H)] if p210 else planes, [((B, 3, H, W), DTYPES[dt])], call)
    return make


def e_rgb_to_ycbcr(p210):
    def make(dt, B, pin, pout):
        H, W = HW
        depth, align, sub = ycbcr_format(p210)
        fmt, codes = _ffi.ycbcr_codes(depth, align, sub, "bt2020", "limited", "center")
        Hc, Wc = ycbcr_ref.chroma_hw(H, W, sub)

        def call(i, o):
            y, cb, cr = frame_pairs(o[0], H, 2) if p210 else o
            _ffi.rgb_to_ycbcr(i[0], ELEM[dt], y, cb, cr, *fmt, B, H, W, *codes, stream())

        outs = [((B, 1, H + Hc, W), torch.int16)] if p210 else [((B, 1, H, W), torch.uint8)] + [((B, 1, Hc, Wc), torch.uint8)] * 2
        return Run([image(dt, B, H, W)], outs, call)
    return make


def e_resize(enlarge):
    def make(dt, B, pin, pout):
        (Hi, Wi), (Ho, Wo) = resize_util.UP3 if enlarge else resize_util.RAGGED
        if pin or pout:  # 18 rows on the far side, the other side in the case's ratio
            Hi, Ho = (18, 18) if pin and pout else (18, 54 if enlarge else 9) if pin else (6 if enlarge else 36, 18)
        need = _ffi.resize_workspace_bytes(Hi, Wi, Ho, Wo, 0)

        def call(i, o):
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")  # NaN in every type, as tests/test_resize_gpu.py
            _ffi.resize(*i[0], *o[0], ELEM[dt], B, Hi, Wi, Ho, Wo, 0, 1, None, ws.data_ptr(), need, stream())

        return Run([image(dt, B, Hi, Wi)], [((B, 3, Ho, Wo), DTYPES[dt])], call)
    return make


def e_interp(mode):
    def make(dt, B, pin, pout):
        (Hi, Wi), (Ho, Wo) = interp_util.RAGGED_UP
        if pin or pout:  # the window below has Ho - 2 rows
            Hi, Ho = (18, 20) if pin and pout else (18, 36) if pin else (10, 20)
        window = (1, 3, Ho - 2, Wo - 4)
        return Run([image(dt, B, Hi, Wi)], [((B, 3, Ho - 2, Wo - 4), DTYPES[dt])],
                   lambda i, o: _ffi.interpolate(*i[0], *o[0], ELEM[dt], B, Hi, Wi, Ho, Wo, mode, int(mode != 0), window, stream()))
    return make


def degrade_entry(what):
    def make(dt, B, pin, pout):
        H, W = rows(37, pin, pout), 45
        need = _ffi.jpeg_workspace_bytes(B, H, W) if what == "jpeg" else 0

        def call(i, o):
            if what == "blur":
                _ffi.blur(*i[0], *o[0], ELEM[dt], B, H, W, 1.0, stream())
            elif what == "noise":
                _ffi.noise(*i[0], *o[0], ELEM[dt], B, H, W, 0.1, 1234, 5, stream())
            else:
                ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
                _ffi.jpeg(*i[0], *o[0], ELEM[dt], B, H, W, 50, ws.data_ptr(), need, stream())

        return Run([image(dt, B, H, W)], [((B, 3, H, W), DTYPES[dt])], call)
    return make


def e_dihedral(k):
    def make(dt, B, pin, pout):
        turned = bool(k & 4)
        H, W = rows(37, pin, pout and not turned), rows(45, pout and turned)
        return Run([image(dt, B, H, W)], [((B, 3, W, H) if turned else (B, 3, H, W), DTYPES[dt])],
                   lambda i, o: _ffi.dihedral(*i[0], *o[0], ELEM[dt], B, H, W, k, stream()))
    return make


def e_ensemble_add(dt, B, pin, pout):
    H, W = 37, rows(45, pin)  # the results below arrive turned: [B, 3, W, H]
    need = _ffi.ensemble_workspace_bytes(B, H, W)

    def call(i, o):
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        _ffi.ensemble_add(*i[0], ELEM[dt], B, H, W, 6, True, ws.data_ptr(), need, stream())
        _ffi.ensemble_add(*i[1], ELEM[dt], B, H, W, 5, False, ws.data_ptr(), need, stream())
        return ws.view(torch.float32).view(B, 3, H, W)

    return Run([image(dt, B, W, H, 5), image(dt, B, W, H, 6)], [], call)


def e_ensemble_finish(dt, B, pin, pout):
    H, W = rows(37, False) if not pout else 36, 45
    need = _ffi.ensemble_workspace_bytes(B, H, W)
    window = (H // 2, W // 3, H - H // 2, W - W // 3)

    def call(i, o):
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        for n, y in enumerate(i):
            _ffi.ensemble_add(*y, ELEM[dt], B, H, W, n, n == 0, ws.data_ptr(), need, stream())
        _ffi.ensemble_finish(*o[0], ELEM[dt], B, H, W, 2, 1, window, ws.data_ptr(), need, stream())

    return Run([image(dt, B, H, W, 5), image(dt, B, H, W, 6)], [((B, 3, window[2], window[3]), DTYPES[dt])], call)


U8_BF16, WITH_F32 = ("u8", "bf16"), ("u8", "bf16", "f32")
# name -> (element types, sides that can be far: "i", "o" or "io", the Run of (dt, B, input side pitched, output side pitched))
ENTRIES = {
    "luma": (WITH_F32, "io", e_luma),
    "metrics_luma": (U8_BF16, "i", metrics_entry(True)),
    "metrics": (U8_BF16, "i", metrics_entry(False)),
    "yuv420_to_rgb-planar": (U8_BF16, "io", e_yuv_to_rgb(False)),
    "yuv420_to_rgb-nv12": (U8_BF16, "io", e_yuv_to_rgb(True)),
    "rgb_to_yuv420-planar": (U8_BF16, "io", e_rgb_to_yuv(False)),
    "rgb_to_yuv420-nv12": (U8_BF16, "io", e_rgb_to_yuv(True)),
    "ycbcr_to_rgb-8bit-420": (WITH_F32, "io", e_ycbcr_to_rgb(False)),
    "ycbcr_to_rgb-10bit-high-422-pairs": (WITH_F32, "io", e_ycbcr_to_rgb(True)),
    "rgb_to_ycbcr-8bit-420": (WITH_F32, "io", e_rgb_to_ycbcr(False)),
    "rgb_to_ycbcr-10bit-high-422-pairs": (WITH_F32, "io", e_rgb_to_ycbcr(True)),
    "resize-bicubic-enlarging": (U8_BF16, "io", e_resize(True)),
    "resize-bicubic-shrinking": (U8_BF16, "io", e_resize(False)),
    "interpolate-bicubic-window": (U8_BF16, "io", e_interp(2)),
    "interpolate-nearest-window": (U8_BF16, "io", e_interp(0)),
    "blur": (U8_BF16, "io", degrade_entry("blur")),
    "noise": (U8_BF16, "io", degrade_entry("noise")),
    "jpeg": (U8_BF16, "io", degrade_entry("jpeg")),
    "dihedral-k1": (U8_BF16, "io", e_dihedral(1)),
    "dihedral-k4": (U8_BF16, "io", e_dihedral(4)),
    "dihedral-k6": (U8_BF16, "io", e_dihedral(6)),
    "ensemble_add": (U8_BF16, "i", e_ensemble_add),
    "ensemble_finish-window": (U8_BF16, "o", e_ensemble_finish),
}
CASES = [(name, dt) for name, (dts, _, _) in ENTRIES.items() for dt in dts]


def is_pitch(km):
    return km is not None and km[0].startswith("pitch")


def run_on(run, kin, kout, index=0):
    """one call of the entry: inputs far as kin says, outputs far as kout says.  -> (what each output view holds, the call's own result)"""
    ins = [place(t, kin if not run.one_far or n == index % len(run.ins) else None) for n, t in enumerate(run.ins)]
    outs = [place(torch.empty(shape, dtype=dtype), kout, write=False) for shape, dtype in run.outs]
    kept = [bits(v.read()).clone() for v in ins]
    res = run.call([v.pair for v in ins], [v.pair for v in outs])
    torch.cuda.synchronize()
    for v, before in zip(ins, kept):
        v.check_guards()
        assert torch.equal(bits(v.read()), before), "the call changed an input"
    for v in outs:
        v.check_guards()
    return [v.read() for v in outs], res


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("name, dt", CASES, ids=lambda v: str(v))
def test_far_views_give_the_bits_of_dense_tensors(name, dt):
    _, sides, make = ENTRIES[name]
    torch.cuda.reset_peak_memory_stats()
    started = time.perf_counter()
    dense = {}
    ran = 0
    for index, (kin, kout) in enumerate(VARIANTS):
        if (kin and "i" not in sides) or (kout and "o" not in sides):
            continue
        B = 2 if all(km is None or km[0].startswith("image") for km in (kin, kout)) else 1
        key = (B, is_pitch(kin), is_pitch(kout))
        run = make(dt, *key)
        if key not in dense:
            dense[key] = run_on(run, None, None)
            again = run_on(run, None, None)
            assert all(same(a, b) for a, b in zip(dense[key][0], again[0])), "two dense runs differ"
        want_outs, want_res = dense[key]
        got_outs, got_res = run_on(run, kin, kout, index)
        for n, (got, want) in enumerate(zip(got_outs, want_outs)):
            if not same(got, want):
                bad = (bits(got) != bits(want)).nonzero()
                raise AssertionError(f"{name} {dt}, inputs {kin}, outputs {kout}: output {n} differs from the dense run's at {bad.shape[0]} of "
                                     f"{got.numel()} elements; first at {tuple(int(v) for v in bad[0])}")
        if want_res is not None:
            assert same(got_res, want_res), f"{name} {dt}, inputs {kin}: the result differs from the dense run's: {got_res} against {want_res}"
        ran += 1
        del got_outs, got_res
    assert ran >= 10
    peak = torch.cuda.max_memory_allocated()
    print(f"far views {name} {dt}: {ran} variants in {time.perf_counter() - started:.2f} s, peak device memory {peak / 1e9:.2f} GB")
    assert peak < fu.MAX_DEVICE_BYTES


@pytest.mark.parametrize("dt", U8_BF16)
def test_noise_in_place_on_a_far_view(dt):
    make = ENTRIES["noise"][2]
    for kind, misalign in KM:
        B = 2 if kind.startswith("image") else 1
        run = make(dt, B, kind.startswith("pitch"), kind.startswith("pitch"))
        (want,), _ = run_on(run, None, None)
        v = place(run.ins[0], (kind, misalign))
        run.call([v.pair], [v.pair])
        torch.cuda.synchronize()
        v.check_guards()
        assert same(v.read(), want), (kind, misalign)


# ---- read views with strides of 0 ----------------------------------------------------------------------------------------------------------
def zero_stride_ins(run, which):
    """(pairs of views that read ONE stored plane of one image through a channel and an image stride of 0, the expanded dense tensors)"""
    pairs, dense, keep = [], [], []
    for n, t in enumerate(run.ins):
        if n in which:
            small = t[:1, :1].contiguous().cuda()
            keep.append(small)
            pairs.append((small.data_ptr(), (0, 0, small.stride(2), small.stride(3))))
            dense.append(small.expand(t.shape).contiguous())
        else:
            dense.append(t.cuda())
            pairs.append(_ffi.pair(dense[-1]))
    return pairs, dense, keep


# entry -> the inputs that are read through strides of 0 (of the *_to_rgb entries: the chroma planes)
ZERO = {"luma": (0,), "metrics_luma": (0, 1), "metrics": (0, 1), "yuv420_to_rgb-planar": (1, 2), "ycbcr_to_rgb-8bit-420": (1, 2),
        "resize-bicubic-enlarging": (0,), "resize-bicubic-shrinking": (0,), "interpolate-bicubic-window": (0,), "interpolate-nearest-window": (0,),
        "blur": (0,), "noise": (0,), "jpeg": (0,), "dihedral-k1": (0,), "dihedral-k6": (0,), "ensemble_add": (0, 1)}


@pytest.mark.parametrize("dt", U8_BF16)
@pytest.mark.parametrize("name", sorted(ZERO))
def test_read_views_with_strides_of_zero(name, dt):
    B = 2
    run = ENTRIES[name][2](dt, B, False, False)
    pairs, dense, keep = zero_stride_ins(run, ZERO[name])

    def go(ins):
        outs = [torch.full(shape, fill_value(dtype), dtype=dtype, device="cuda") for shape, dtype in run.outs]
        res = run.call(ins, [_ffi.pair(o) for o in outs])
        torch.cuda.synchronize()
        return outs + ([res] if res is not None else [])

    want, got = go([_ffi.pair(t) for t in dense]), go(pairs)
    assert len(want) > 0 and all(same(a, b) for a, b in zip(got, want)), name


# ---- mz_forward_view: a far input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", U8_BF16)
def test_upscale_into_reads_a_far_input_view(dt):
    m = lower_built("g1", torch.bfloat16)  # g1_2x_c16; a uint8 call runs the bf16 engine
    torch.cuda.reset_peak_memory_stats()
    for kind, misalign in [km for km in KM if not km[0].endswith("_neg")]:
        B, H, W = (2 if kind == "image" else 1), (fu.PITCH_H if kind == "pitch" else 33), 45
        x = image(dt, B, H, W)
        x = x if dt == "u8" else x.float().clamp(0, 1).to(x.dtype)
        want = torch.empty((B, 3, 2 * H, 2 * W), dtype=x.dtype, device="cuda")
        m.upscale_into(x.cuda(), want)
        v = fu.far_view(x, kind, misalign, device="cuda")
        got = torch.full_like(want, fill_value(want.dtype))
        m.upscale_into(v.tv, got)
        torch.cuda.synchronize()
        v.check_guards()
        assert same(got, want) and same(v.read(), x.cuda()), (kind, misalign)
    assert torch.cuda.max_memory_allocated() < fu.MAX_DEVICE_BYTES
