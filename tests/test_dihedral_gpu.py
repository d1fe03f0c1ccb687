"""mz_dihedral, mz_ensemble_add and mz_ensemble_finish on the GPU against the torch restatement of tests/ensemble_ref.py, bit for bit.

The transform moves elements: its inputs are RANDOM BIT PATTERNS of the element's width (NaN with every payload, -0, infinities and
denormals among them, and planted by hand as well) and the comparison is on the bits.  The accumulator arithmetic is float32 adds in call
order and one finish; torch's float32 add, multiply by a power of two and cast round as the device does, so those are equalities too.
Shapes: one pixel, one row, one column, a ragged multi-tile image, exactly one tile, tiles with ragged edges on both axes, a short wide
one.  Layouts at both ends: dense (the 16-byte path where the width allows it), channels-last, a crop at an odd element offset, rows
padded to an aligned pitch (flipped tiles start misaligned: both paths inside one launch), a transposed view (unit ROW stride), and --
through _ffi -- a negative channel stride."""

import pytest
import torch

import ensemble_ref as ref
from ensemble_ref import DTYPES, INT_OF, pass_results, random_bits, shape_id, stream
from ultrazoom_amd import _ffi, dihedral

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 31, 33), (1, 64, 64), (2, 65, 127), (1, 8, 200)]
SENTINEL = 0x5A


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert torch.equal(ref.bits(got), ref.bits(want)), what


def crop(t: torch.Tensor, top=2, left=3, bottom=3, right=3):
    """t's pixels as a crop of a larger frame that starts ONE element into its allocation: rows begin at odd element offsets.
    -> (the frame's flat buffer as bytes, the crop)"""
    B, C, H, W = t.shape
    fh, fw = H + top + bottom, W + left + right
    flat = torch.empty(B * C * fh * fw + 1, dtype=t.dtype, device=t.device)
    flat.view(torch.uint8).fill_(SENTINEL)
    view = flat[1:].view(B, C, fh, fw)[:, :, top : top + H, left : left + W]
    view.copy_(t)
    return flat.view(torch.uint8), view


def padded(t: torch.Tensor):
    """t's pixels in rows padded to a pitch of a multiple of 16 elements: an aligned base and aligned strides whatever W is."""
    B, C, H, W = t.shape
    pitch = (W + 15) // 16 * 16 + 16
    frame = torch.empty(B, C, H, pitch, dtype=t.dtype, device=t.device)
    frame.view(torch.uint8).fill_(SENTINEL)
    view = frame[:, :, :, :W]
    view.copy_(t)
    return frame.view(torch.uint8), view


def nothing_outside(frame_bytes: torch.Tensor, view: torch.Tensor) -> bool:
    """Call it LAST: overwrites the view's elements with sentinel bytes; the whole frame is then sentinel unless a store went astray."""
    size = view.element_size()
    view.view(INT_OF[size]).fill_(int.from_bytes(bytes([SENTINEL]) * size, "little"))
    return bool((frame_bytes == SENTINEL).all())


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_dihedral_moves_bit_patterns(shape, dt):
    B, H, W = shape
    x = random_bits(dt, B, H, W)
    for k in range(8):
        want = ref.T(x, k).contiguous()
        # dense
        assert_same_bits(dihedral(x, k), want, ("dense", k))
        # channels-last at both ends
        out = torch.empty_like(want, memory_format=torch.channels_last)
        assert dihedral(x.contiguous(memory_format=torch.channels_last), k, out=out) is out
        assert_same_bits(out, want, ("channels-last", k))
        # a crop of a larger frame at an odd element offset, at both ends
        _, xc = crop(x)
        frame, oc = crop(torch.zeros_like(want))
        dihedral(xc, k, out=oc)
        assert_same_bits(oc, want, ("crop", k))
        assert nothing_outside(frame, oc), ("crop: stores outside", k)
        # rows padded to an aligned pitch: a column flip starts its interior tiles misaligned
        _, xp = padded(x)
        frame, op = padded(torch.zeros_like(want))
        dihedral(xp, k, out=op)
        assert_same_bits(op, want, ("padded", k))
        assert nothing_outside(frame, op), ("padded: stores outside", k)
        # a transposed tensor as the input: its unit stride is the ROW stride
        xt = x.transpose(2, 3).contiguous().transpose(2, 3)
        assert xt.stride(2) == 1 or W == 1 or H == 1
        assert_same_bits(dihedral(xt, k), want, ("transposed view", k))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(3, 31, 33), (2, 65, 127)], ids=shape_id)
def test_dihedral_reads_a_negative_channel_stride_as_bgr(shape, dt):
    B, H, W = shape
    x = random_bits(dt, B, H, W)
    for k in (0, 3, 5, 6):
        want = ref.T(x.flip(1), k).contiguous()
        out = torch.empty_like(want)
        s = x.stride()
        _ffi.dihedral(x[:, 2].data_ptr(), (s[0], -s[1], s[2], s[3]), out.data_ptr(), out.stride(), _ffi.elem_code(x.dtype), B, H, W, k, stream())
        assert_same_bits(out, want, ("negative channel stride in", k))
        # ... and at the output: written back to front, the tensor holds T(x, k)
        out2 = torch.empty_like(want)
        so = out2.stride()
        _ffi.dihedral(x[:, 2].data_ptr(), (s[0], -s[1], s[2], s[3]), out2[:, 2].data_ptr(), (so[0], -so[1], so[2], so[3]),
                      _ffi.elem_code(x.dtype), B, H, W, k, stream())
        assert_same_bits(out2, ref.T(x, k).contiguous(), ("negative channel stride at both ends", k))


def test_dihedral_round_trip_and_the_python_refusals():
    x = random_bits("bf16", 2, 65, 127)
    for k in range(8):
        assert_same_bits(dihedral(dihedral(x, k), ref.inverse(k)), x, k)
    with pytest.raises(ValueError, match="0..7"):
        dihedral(x, 8)
    with pytest.raises(ValueError, match="expected the one shape"):
        dihedral(x, 4, out=torch.empty_like(x))
    with pytest.raises(_ffi.MewZoomHipError, match="overlap"):
        dihedral(x, 3, out=x)


# ---- the accumulator ---------------------------------------------------------------------------------------------------------------
ORDERS = {1: [5], 2: [6, 0], 4: [3, 7, 4, 1], 8: [2, 5, 0, 7, 1, 6, 3, 4]}  # call orders: every k, as first and as a later add


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_add_and_finish_are_the_stated_arithmetic(shape, dt):
    B, H, W = shape
    dtype, elem = DTYPES[dt], _ffi.elem_code(DTYPES[dt])
    ys = pass_results(dt, B, H, W)
    need = _ffi.ensemble_workspace_bytes(B, H, W)
    assert need == 12 * B * H * W
    ties = 0
    for n, order in ORDERS.items():
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")  # NaN as float32: the first add stores
        acc = ws.view(torch.float32).view(B, 3, H, W)
        for i, k in enumerate(order):
            y = ys[k]
            if i % 2:  # every second result arrives channels-last
                y = y.contiguous(memory_format=torch.channels_last)
            _ffi.ensemble_add(y.data_ptr(), y.stride(), elem, B, H, W, k, i == 0, ws.data_ptr(), need, stream())
            want_acc = ref.accumulate([ys[j] for j in order[: i + 1]], order[: i + 1])
            assert torch.equal(ref.bits(acc), ref.bits(want_acc)), (n, i, k)
        if dt == "u8":
            ties += int(((2 * want_acc.to(torch.int64)) % (2 * n) == n).sum())
        kept = acc.clone()
        for clamp in (False, True):
            want = ref.finish(want_acc, n, dtype, clamp)
            out = torch.empty((B, 3, H, W), dtype=dtype, device="cuda")
            _ffi.ensemble_finish(out.data_ptr(), out.stride(), elem, B, H, W, n, clamp, None, ws.data_ptr(), need, stream())
            assert_same_bits(out, want, ("finish", n, clamp))
            strided = torch.empty((B, 3, H, W), dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)
            _ffi.ensemble_finish(strided.data_ptr(), strided.stride(), elem, B, H, W, n, clamp, None, ws.data_ptr(), need, stream())
            assert_same_bits(strided, want, ("finish, channels-last", n, clamp))
            for window in {(0, 0, H, W), (H // 2, W // 3, H - H // 2, W - W // 3), (0, W // 2, max(1, H // 2), 1)}:
                y0, x0, h, w = window
                frame, part = crop(torch.zeros((B, 3, h, w), dtype=dtype, device="cuda"))
                _ffi.ensemble_finish(part.data_ptr(), part.stride(), elem, B, H, W, n, clamp, window, ws.data_ptr(), need, stream())
                assert_same_bits(part, want[:, :, y0 : y0 + h, x0 : x0 + w].contiguous(), ("finish, window", n, clamp, window))
                assert nothing_outside(frame, part), ("finish: stores outside the window", window)
        assert torch.equal(ref.bits(acc), ref.bits(kept)), "finish does not write the accumulator"
    if dt == "u8" and B * H * W >= 64:
        assert ties > 0, "no sum landed on a rounding tie"


def test_the_uint8_finish_rounds_half_up_at_every_sum():
    """Every sum 0 .. 255 n of n = 1, 2, 4, 8 samples, through add (two results whose samples add up to it) and finish."""
    for n in (1, 2, 4, 8):
        sums = torch.arange(0, 255 * n + 1, device="cuda")
        W = sums.numel()
        parts = [torch.clamp(sums - 255 * i, 0, 255).to(torch.uint8) for i in range(n)]  # part i takes what the earlier ones left
        assert torch.equal(sum(p.to(torch.int64) for p in parts), sums)
        need = _ffi.ensemble_workspace_bytes(1, 1, W)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        for i, p in enumerate(parts):
            y = p.view(1, 1, 1, W).expand(1, 3, 1, W)  # (a channel stride of 0: views that are only read may have one)
            _ffi.ensemble_add(y.data_ptr(), y.stride(), 3, 1, 1, W, 0, i == 0, ws.data_ptr(), need, stream())
        out = torch.empty((1, 3, 1, W), dtype=torch.uint8, device="cuda")
        _ffi.ensemble_finish(out.data_ptr(), out.stride(), 3, 1, 1, W, n, 1, None, ws.data_ptr(), need, stream())
        want = ((2 * sums + n) // (2 * n)).to(torch.uint8)
        assert torch.equal(out[0, 1, 0], want) and torch.equal(out[0, 0], out[0, 2])
        halves = sums[(2 * sums) % (2 * n) == n]
        assert n == 1 or (halves.numel() > 0 and torch.equal(want[halves].to(torch.int64), (halves + n // 2) // n))  # ties go up


# ---- past 2^32 elements ------------------------------------------------------------------------------------------------------------
def test_dihedral_past_two_to_the_32_elements():
    """uint8 [1, 3, 37000, 39000] = 4.33e9 elements, k = 7 (both flips and the transposition): every element offset of the kernel is
    64-bit.  About 13 GB of tensors: the input, the output and the chunks of the comparison."""
    H, W = 37000, 39000
    n = 3 * H * W
    assert n > 1 << 32
    free, _ = torch.cuda.mem_get_info()
    if free < 14 * (1 << 30):
        pytest.skip(f"needs 14 GB of free device memory, {free / 2**30:.1f} GB are free")
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.empty((1, 3, H, W), dtype=torch.uint8, device="cuda")
    for c in range(3):  # (no call spans 2^32 elements)
        x[0, c].random_(0, 256, generator=g)
    out = dihedral(x, 7)
    assert out.shape == (1, 3, W, H)
    want = ref.T(x, 7)
    rows = 3000
    for r0 in range(0, W, rows):
        assert torch.equal(out[:, :, r0 : r0 + rows], want[:, :, r0 : r0 + rows]), f"output rows {r0}.."
    # the far corners by hand: out[c, i, j] = x[c, H - 1 - j, W - 1 - i]
    for c, i, j in ((0, 0, 0), (2, W - 1, H - 1), (1, 12345, 36999), (2, 38999, 1)):
        assert int(out[0, c, i, j]) == int(x[0, c, H - 1 - j, W - 1 - i])
    del out, want, x
    torch.cuda.empty_cache()
