"""The resampling kernel (mz_resize, ultrazoom_amd/resize.py) against torch's own antialiased interpolate in float64 on the CPU.  Inputs
are uniform noise (the hardest case for a bicubic: it overshoots to about -0.12 .. 1.13) rounded to the element type first, so both
sides see the same values.

Gates (the kernel accumulates both passes in float64, the intermediate is float32):
  f32        max-abs <= 1e-5
  bf16, f16  |got - want64| <= one ulp of the storage type at want64
  uint8      equal to floor(clamp(want64, 0, 1) 255 + 0.5), except where 255 want64 lies within 1e-3 of a tie: there at most 1 LSB, and
             those elements are fewer than 1 %.  Measured on the CPU with the float64 checker alone and the seeds below: at most 0.6 %,
             EXACT ties aside.  An exact tie -- 255 want64 = k + 1/2 in rational arithmetic, the checker within 1e-9 of it -- is no
             matter of the seed: the bilinear weights are small fractions (k / 8 at x1/2, k / 6 at x3/4 ..) and the pixels integers, so
             4.9 % of the 48x64 -> 36x48 results and 1.8 % of the 34x190 -> 17x95 ones are ties by construction (bicubic: 0.07 % at x3, else
             none).  The definition has no single answer there, so exact ties are allowed their 1 LSB without counting towards the 1 %;
             every case stays in, and every element that is not within 1e-3 of a tie must be equal.
Everything else is an equality: windows, batches, layouts, repeated calls, a poisoned workspace."""

from functools import lru_cache

import pytest
import torch

from resize_util import DTYPES, ELEM, FILTERS, RAGGED, TAPS66, TILE_H, TILE_W, UP3, assert_within_gate, hip_resize, image, model_and_input, shape_id, want64_of
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

SHAPES = [((64, 80), (16, 20)), ((37, 45), (12, 15)), ((48, 64), (36, 48)), ((33, 47), (11, 13)), UP3, ((41, 41), (41, 17)),
          ((64, 64), (9, 7)), ((17, 19), (2, 3)), TAPS66, RAGGED]
@lru_cache(maxsize=None)
def checker(B: int, shape, dt: str, filt: str) -> torch.Tensor:
    """The checker, once per case"""
    return want64_of(image(B, *shape[0], dt), shape[1], filt)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_against_torchs_float64_interpolate(shape, dt, filt):
    for B in (1, 3):
        x = image(B, *shape[0], dt)
        got = hip_resize(x.cuda(), shape[1], filter=filt)
        assert_within_gate(got, checker(B, shape, dt, filt), dt, f"{shape_id(shape)} B={B} {dt} {filt}")


# the lower edge: one pixel in, one pixel out, a single row, a single column, every tap clamped to one or two pixels
SMALL_SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((1, 7), (2, 3)), ((5, 1), (2, 1)), ((16, 16), (1, 1)), ((2, 2), (7, 9))]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=shape_id)
def test_the_smallest_shapes_against_torchs_float64_interpolate(shape, dt, filt):
    for B in (1, 3):
        x = image(B, *shape[0], dt)
        got = hip_resize(x.cuda(), shape[1], filter=filt)
        assert_within_gate(got, checker(B, shape, dt, filt), dt, f"{shape_id(shape)} B={B} {dt} {filt}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("filt", FILTERS)
def test_same_size_gives_the_input(filt, dt):
    x = image(2, 41, 41, dt).cuda()
    assert torch.equal(hip_resize(x, (41, 41), filter=filt), x)
    # one identity axis: that axis adds nothing to the other one's result
    tall = hip_resize(x, (41, 17), filter=filt)
    assert tall.shape == (2, 3, 41, 17)
    assert_within_gate(tall, want64_of(x, (41, 17), filt), dt, f"41x41to41x17 {dt} {filt}")


@pytest.mark.parametrize("dt", ["bf16", "u8"])
def test_two_calls_and_single_images_give_the_same_bits(dt):
    (hin, win), size = RAGGED
    x = image(3, hin, win, dt).cuda()
    first, second = hip_resize(x, size), hip_resize(x, size)
    assert torch.equal(first, second)
    for b in range(3):
        assert torch.equal(hip_resize(x[b:b + 1], size)[0], first[b]), b


WINDOWS = {"inside one tile": (TILE_H + 2, TILE_W + 3, 3, 5), "across tile edges": (TILE_H - 3, TILE_W - 5, TILE_H + 4, 2 * TILE_W + 1),
           "last row and column": (2 * TILE_H, 3 * TILE_W - 2, 1, 1), "last rows and columns": (TILE_H + 1, 2 * TILE_W - 1, TILE_H, TILE_W),
           "everything": (0, 0, 2 * TILE_H + 1, 3 * TILE_W - 1)}


@pytest.mark.parametrize("dt", ["f32", "bf16", "u8"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_a_window_is_that_part_of_the_whole_result(name, dt):
    (hin, win), size = RAGGED
    y0, x0, h, w = WINDOWS[name]
    x = image(2, hin, win, dt).cuda()
    whole = hip_resize(x, size)
    part = hip_resize(x, size, window=(y0, x0, h, w))
    assert part.shape == (2, 3, h, w)
    assert torch.equal(part, whole[:, :, y0:y0 + h, x0:x0 + w])
    # ... and of the 3x enlargement and the 66-tap reduction
    for (src, dst), win_ in ((UP3, (30, 50, 20, 40)), (TAPS66, (7, 30, 3, 10))):
        x = image(1, *src, dt).cuda()
        assert torch.equal(hip_resize(x, dst, window=win_), hip_resize(x, dst)[:, :, win_[0]:win_[0] + win_[2], win_[1]:win_[1] + win_[3]])


def raw(x_ptr, x_strides, out, elem, B, hin, win, size, filt=0, clamp=0, window=None, fill=None):
    """mz_resize on raw views (negative strides, which torch tensors cannot express), on a workspace of `fill` bytes"""
    need = _ffi.resize_workspace_bytes(hin, win, size[0], size[1], filt)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    _ffi.resize(x_ptr, x_strides, out.data_ptr(), out.stride(), elem, B, hin, win, size[0], size[1], filt, clamp, window, ws.data_ptr(), need,
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", ["f32", "u8"])
def test_a_nan_filled_workspace_gives_the_same_bits(dt):
    for (hin, win), size in (RAGGED, TAPS66, UP3):
        x = image(2, hin, win, dt).cuda()
        want = hip_resize(x, size)
        got = raw(x.data_ptr(), x.stride(), torch.empty_like(want), ELEM[dt], 2, hin, win, size, fill=0xFF)
        assert torch.equal(got, want)


VIEWS = ["channels_last", "hwc_frame", "crop", "every_second_image"]


@pytest.mark.parametrize("dt", ["bf16", "u8", "f32"])
@pytest.mark.parametrize("kind", VIEWS)
def test_input_views_give_the_bits_of_a_dense_copy(kind, dt):
    B, (H, W), size = 2, (37, 45), (12, 15)
    x = image(B, H, W, dt).cuda()
    dense = hip_resize(x, size)
    if kind == "channels_last":
        v = x.contiguous(memory_format=torch.channels_last)
        assert v.stride() == (3 * H * W, 1, 3 * W, 3)
    elif kind == "hwc_frame":
        v = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    elif kind == "crop":
        big = torch.full((B, 3, H + 7, W + 9), float("nan") if dt != "u8" else 255, device="cuda").to(x.dtype)
        big[:, :, 3:3 + H, 5:5 + W] = x
        v = big[:, :, 3:3 + H, 5:5 + W]
    else:
        big = torch.full((2 * B, 3, H, W), float("nan") if dt != "u8" else 255, device="cuda").to(x.dtype)
        big[::2] = x
        v = big[::2]
    assert not v.is_contiguous() and torch.equal(v, x)
    assert torch.equal(hip_resize(v, size), dense), kind


@pytest.mark.parametrize("dt", ["bf16", "u8"])
@pytest.mark.parametrize("kind", ["channels_last", "hwc_frame", "crop_of_a_canvas", "every_second_image"])
def test_output_views_are_written_in_place_and_nothing_else(kind, dt):
    B, (H, W), size = 2, (37, 45), (12, 15)
    x = image(B, H, W, dt).cuda()
    dense = hip_resize(x, size)
    mark = 77 if dt == "u8" else 0.4375

    def view_of(canvas):
        if kind == "hwc_frame":
            return canvas.permute(0, 3, 1, 2)
        if kind == "crop_of_a_canvas":
            return canvas[:, :, 2:2 + size[0], 7:7 + size[1]]
        return canvas[1::2] if kind == "every_second_image" else canvas

    shape = {"channels_last": (B, 3) + size, "hwc_frame": (B,) + size + (3,), "crop_of_a_canvas": (B, 3, size[0] + 6, size[1] + 10),
             "every_second_image": (2 * B, 3) + size}[kind]
    canvas = torch.full(shape, mark, device="cuda").to(x.dtype)
    if kind == "channels_last":
        canvas = canvas.contiguous(memory_format=torch.channels_last)
    want = canvas.clone()
    view_of(want).copy_(dense)
    out = view_of(canvas)
    got = hip_resize(x, size, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, dense)
    assert torch.equal(canvas, want), "bytes outside the output view changed"
    # a window of the result into a crop of a canvas
    canvas = torch.full((B, 3, 20, 20), mark, device="cuda").to(x.dtype)
    before = canvas.clone()
    hip_resize(x, size, out=canvas[:, :, 4:9, 6:13], window=(5, 3, 5, 7))
    assert torch.equal(canvas[:, :, 4:9, 6:13], dense[:, :, 5:10, 3:10])
    canvas[:, :, 4:9, 6:13] = before[:, :, 4:9, 6:13]
    assert torch.equal(canvas, before)


@pytest.mark.parametrize("dt", ["bf16", "u8"])
def test_bgr_through_a_negative_channel_stride(dt):
    B, (H, W), size = 2, (37, 45), (12, 15)
    x = image(B, H, W, dt).cuda()
    dense = hip_resize(x, size)
    frame = x.flip(1).permute(0, 2, 3, 1).contiguous()  # [B, H, W, 3] holding B, G, R
    got = raw(frame.data_ptr() + 2 * frame.element_size(), (H * W * 3, -1, W * 3, 3), torch.empty_like(dense), ELEM[dt], B, H, W, size)
    assert torch.equal(got, dense)
    # and on the output side: an RGB image stored into a BGR frame
    out_frame = torch.zeros((B,) + size + (3,), device="cuda").to(x.dtype)
    ov = _ffi.MzImageView(out_frame.data_ptr() + 2 * out_frame.element_size(), (_ffi.c_int64 * 4)(size[0] * size[1] * 3, -1, size[1] * 3, 3))
    need = _ffi.resize_workspace_bytes(H, W, size[0], size[1], 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    xv = _ffi.MzImageView(x.data_ptr(), (_ffi.c_int64 * 4)(*x.stride()))
    _ffi.check(_ffi.lib().mz_resize(_ffi.byref(xv), _ffi.byref(ov), ELEM[dt], B, H, W, size[0], size[1], 0, 0, None, ws.data_ptr(), need,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out_frame.permute(0, 3, 1, 2).flip(1), dense)


def test_clamp_clamps_the_overshoot_of_the_3x_bicubic():
    x = image(1, 24, 40, "f32").cuda()
    free = hip_resize(x, (72, 120))
    held = hip_resize(x, (72, 120), clamp=True)
    print("3x bicubic of uniform noise spans", float(free.min()), float(free.max()))
    assert float(free.min()) < -0.02 and float(free.max()) > 1.02
    assert float(held.min()) == 0.0 and float(held.max()) == 1.0
    assert torch.equal(held, free.clamp(0, 1))
    assert_within_gate(free, checker(1, UP3, "f32", "bicubic"), "f32", "3x bicubic, clamp=False")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_constant_image_stays_constant(dt):
    value = 0.3
    for (hin, win), size in (((64, 80), (16, 20)), UP3, TAPS66, ((48, 64), (36, 48))):
        x = torch.full((1, 3, hin, win), value)
        x = (x * 255).round().to(torch.uint8) if dt == "u8" else x.to(DTYPES[dt])
        for filt in FILTERS:
            assert_within_gate(hip_resize(x.cuda(), size, filter=filt), want64_of(x, size, filt), dt, f"constant {hin}x{win} {dt} {filt}")


def test_the_c_entry_refuses_what_the_python_layer_refuses():
    x = image(1, 37, 45, "f32").cuda()
    with pytest.raises(ValueError, match="16"):
        hip_resize(x, (2, 15))
    with pytest.raises(ValueError, match="window"):
        hip_resize(x, (12, 15), window=(10, 0, 3, 3))
    with pytest.raises(TypeError, match="same dtype"):
        hip_resize(x, (12, 15), out=torch.empty((1, 3, 12, 15), dtype=torch.float16, device="cuda"))
    with pytest.raises(_ffi.MewZoomHipError):
        raw(x.data_ptr(), x.stride(), torch.empty((1, 3, 2, 15), device="cuda"), 0, 1, 37, 45, (2, 15))
    assert_within_gate(hip_resize(x, (12, 15)), want64_of(x, (12, 15), "bicubic"), "f32", "after the refusals")


# ---- MewZoom.upscale_to ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_upscale_to(dt):
    m, x = model_and_input(dt)
    up = m.upscale(x)
    assert torch.equal(m.upscale_to(x, (96, 160)), up)
    for size in ((72, 120), (48, 80)):
        got = m.upscale_to(x, size)
        assert torch.equal(got, hip_resize(up, size, clamp=True))
        # against the checker applied to the GPU's own upscale(x): the model's parity is not judged again here
        assert_within_gate(got, want64_of(up, size, "bicubic").clamp(0, 1), dt, f"upscale_to {size} {dt}")
        assert torch.equal(m.upscale_to(x, size, filter="bilinear"), hip_resize(up, size, filter="bilinear", clamp=True))
    out = torch.empty((1, 3, 72, 120), dtype=x.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    assert m.upscale_to(x, (72, 120), out=out).data_ptr() == out.data_ptr()
    assert out.stride() == (3 * 72 * 120, 1, 3 * 120, 3) and torch.equal(out, m.upscale_to(x, (72, 120)))
    full = torch.empty((1, 3, 96, 160), dtype=x.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    assert torch.equal(m.upscale_to(x, (96, 160), out=full), up)


def test_upscale_to_with_uint8_images():
    m, x = model_and_input("bf16")
    x8 = (x.float() * 255).round().to(torch.uint8)
    up8 = m.upscale_uint8(x8)
    assert torch.equal(m.upscale_to(x8, (96, 160)), up8)
    for size in ((72, 120), (48, 80)):
        got = m.upscale_to(x8, size)
        assert got.dtype == torch.uint8 and torch.equal(got, hip_resize(up8, size, clamp=True))
        assert_within_gate(got, want64_of(up8, size, "bicubic"), "u8", f"upscale_to {size} uint8")


# ---- evaluation: HR -> LR -> upscale -> metrics on the device ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 52, 68, 4), (1, 45, 70, 2)], ids=["52x68by4", "45x70by2"])
def test_lr_from_hr_on_the_device(case, dt):
    from ultrazoom_amd.evaluate import lr_from_hr

    B, H, W, ratio = case
    hr = image(B, H, W, dt).cuda()
    for filt in FILTERS:
        lr, cropped = lr_from_hr(hr, ratio, filter=filt, backend="hip")
        h, w = H // ratio, W // ratio
        assert lr.shape == (B, 3, h, w) and cropped.shape == (B, 3, h * ratio, w * ratio) and cropped.data_ptr() == hr.data_ptr()
        assert_within_gate(lr, want64_of(hr[:, :, :h * ratio, :w * ratio], (h, w), filt), dt, f"lr_from_hr {case} {dt} {filt}")


def test_evaluate_hr_keeps_the_chain_on_the_device():
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr, lr_from_hr
    from ultrazoom_amd.synth import synth_image

    m, _ = model_and_input("bf16")
    hr = synth_image(2, 97, 130, seed=9).to("cuda", torch.bfloat16)
    got = evaluate_hr(m, [hr], backend="hip")
    want = evaluate(m, [lr_from_hr(hr, m.upscale_ratio, backend="hip")], backend="hip")
    print(got)
    assert got == want and got["images"] == 2 and got["vif"] is not None
    assert 10.0 < got["psnr"] < 60.0
