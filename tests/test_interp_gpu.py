"""The plain-interpolation kernel (mz_interpolate, ultrazoom_amd/interpolate.py) against torch's own interpolate (align_corners=False, no
antialiasing) in float64 on the CPU, and against the model's own skip connection.  Inputs are uniform noise (the hardest case for a
bicubic) rounded to the element type first, so both sides see the same values.

Gates: those of the resampling tests (resize_util.assert_within_gate): f32 max-abs <= 1e-5; bf16, f16 within one ulp of the storage type at
the float64 value; uint8 equal to floor(clamp(want64, 0, 1) 255 + 0.5) except within 1e-3 of a tie (there at most 1 LSB; such elements,
exact ties aside, are fewer than 1 %: the float64 reference alone gives at most 0.39 % at these shapes).  The kernel accumulates both
passes in float64 and rounds once, so the f32 figure is the rounding itself: about 6e-8 at values up to 1.3 (printed by every case).
Nearest is an equality of bit patterns.  Everything else is an equality, too: layouts, windows, batches, repeated calls, the two paths of the kernel."""

import pytest
import torch

from golden_util import GoldenCase
from interp_util import (DTYPES, ELEM, MODE, RAGGED_DOWN, RAGGED_UP, SHAPES, STAGE_ROWS, TILE_H, TILE_W, UP3, assert_within_gate, bits, checker,
                         gate_image, hip_interp, image, nearest_of, shape_id, want64_of)
from ultrazoom_amd import MewZoom, _ffi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_against_torchs_float64_interpolate(shape, dt, mode):
    for B in (1, 3):
        x = gate_image(B, shape, dt)
        got = hip_interp(x.cuda(), shape[1], mode=mode)
        assert_within_gate(got, checker(B, shape, dt, mode), dt, f"{shape_id(shape)} B={B} {dt} {mode}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_nearest_moves_bit_patterns_as_torch_picks_them(shape, dt):
    for B in (1, 3):
        x = image(B, *shape[0], dt)
        got = hip_interp(x.cuda(), shape[1], mode="nearest")
        assert got.dtype == x.dtype and torch.equal(bits(got), bits(nearest_of(x, shape[1]))), (shape, B)


def test_nearest_keeps_nan_payloads_and_negative_zero():
    pattern = torch.tensor([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0xFF800000, 0x3F800000], dtype=torch.int64)
    words = pattern[torch.arange(3 * 9 * 11) % len(pattern)].to(torch.int32).view(1, 3, 9, 11)
    for dt, x in (("f32", words.view(torch.float32)), ("bf16", (words >> 16).to(torch.int16).view(torch.bfloat16)),
                  ("f16", (words >> 16).to(torch.int16).view(torch.float16))):
        for size in ((36, 44), (9, 11), (4, 5)):
            assert torch.equal(bits(hip_interp(x.cuda(), size, mode="nearest")), bits(nearest_of(x, size))), (dt, size)


@pytest.mark.parametrize("r", [2, 4, 8])
def test_scale_factor_is_the_size_form_and_torchs_upsample(r):
    x = image(2, 9, 11, "f32")
    got = hip_interp(x.cuda(), scale_factor=r)
    assert torch.equal(got, hip_interp(x.cuda(), (9 * r, 11 * r)))
    up = torch.nn.Upsample(scale_factor=r, mode="bicubic")(x.double())
    assert torch.equal(up, want64_of(x, (9 * r, 11 * r), "bicubic"))  # torch's two coordinate rules coincide at integer factors
    assert_within_gate(got, up, "f32", f"Upsample x{r}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("mode", sorted(MODE))
def test_same_size_gives_the_input(mode, dt):
    x = image(2, 41, 41, dt).cuda()
    assert torch.equal(hip_interp(x, (41, 41), mode=mode), x)
    if mode != "nearest":  # one identity axis: that axis adds nothing to the other one's result
        for shape in (((41, 41), (41, 17)), ((41, 41), (90, 41))):
            got = hip_interp(gate_image(2, shape, dt).cuda(), shape[1], mode=mode)
            assert_within_gate(got, checker(2, shape, dt, mode), dt, f"{shape_id(shape)} {dt} {mode}")


def test_clamp_clamps_the_overshoot_of_zero_one_data():
    x = (image(1, 24, 40, "f32") > 0.5).float().cuda()
    free = hip_interp(x, scale_factor=4)
    held = hip_interp(x, scale_factor=4, clamp=True)
    print("4x bicubic of 0 / 1 noise spans", float(free.min()), float(free.max()))
    # x4 has the phases t = 1/8, 3/8, 5/8, 7/8; at 3/8 the positive weights of an axis add up to P = 1.17676 and the negative ones to
    # 1 - P, so on 0 / 1 data a result lies in [2 P (1 - P), P^2 + (1 - P)^2] = [-0.416, 1.416]; noise comes close to both ends
    assert -0.4161 < float(free.min()) < -0.25 and 1.25 < float(free.max()) < 1.4161
    assert float(held.min()) == 0.0 and float(held.max()) == 1.0 and torch.equal(held, free.clamp(0, 1))
    for dt in ("bf16", "f16"):
        assert torch.equal(hip_interp(x.to(DTYPES[dt]), scale_factor=4, clamp=True), hip_interp(x.to(DTYPES[dt]), scale_factor=4).clamp(0, 1))


# ---- the same bits ---------------------------------------------------------------------------------------------------------------------
CASES = [(UP3, "bicubic"), (RAGGED_UP, "bilinear"), (((37, 45), (12, 15)), "bicubic"), (((9, 11), (36, 44)), "nearest")]


def case_id(c):
    return f"{shape_id(c[0])}_{c[1]}"


@pytest.mark.parametrize("dt", ["bf16", "u8"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_two_calls_and_single_images_give_the_same_bits(case, dt):
    ((hin, win), size), mode = case
    x = image(3, hin, win, dt).cuda()
    first, second = hip_interp(x, size, mode=mode), hip_interp(x, size, mode=mode)
    assert torch.equal(first, second)
    for b in range(3):
        assert torch.equal(hip_interp(x[b:b + 1], size, mode=mode)[0], first[b]), b


@pytest.mark.parametrize("dt", ["bf16", "u8", "f32"])
@pytest.mark.parametrize("kind", ["channels_last", "hwc_frame", "crop", "every_second_image"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_input_views_give_the_bits_of_a_dense_copy(case, kind, dt):
    ((H, W), size), mode = case
    B = 2
    x = image(B, H, W, dt).cuda()
    dense = hip_interp(x, size, mode=mode)
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
    assert torch.equal(hip_interp(v, size, mode=mode), dense), kind


@pytest.mark.parametrize("dt", ["bf16", "u8", "f32"])
@pytest.mark.parametrize("kind", ["channels_last", "hwc_frame", "crop_of_a_canvas", "every_second_image"])
def test_output_views_are_written_in_place_and_nothing_else(kind, dt):
    B, (H, W), size = 2, (24, 40), (72, 120)
    x = image(B, H, W, dt).cuda()
    dense = hip_interp(x, size)
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
    got = hip_interp(x, size, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, dense)
    assert torch.equal(canvas, want), "bytes outside the output view changed"
    # a window of the result into a crop of a canvas
    canvas = torch.full((B, 3, 20, 20), mark, device="cuda").to(x.dtype)
    before = canvas.clone()
    hip_interp(x, size, out=canvas[:, :, 4:9, 6:13], window=(35, 63, 5, 7))
    assert torch.equal(canvas[:, :, 4:9, 6:13], dense[:, :, 35:40, 63:70])
    canvas[:, :, 4:9, 6:13] = before[:, :, 4:9, 6:13]
    assert torch.equal(canvas, before)


def raw(x_ptr, x_strides, out_ptr, out_strides, elem, B, hin, win, size, mode=2, clamp=0, window=None):
    """mz_interpolate on raw views (negative strides, which torch tensors cannot express)"""
    _ffi.interpolate(x_ptr, x_strides, out_ptr, out_strides, elem, B, hin, win, size[0], size[1], mode, clamp, window,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", ["bf16", "u8"])
def test_bgr_through_a_negative_channel_stride(dt):
    B, (H, W), size = 2, (24, 40), (72, 120)
    x = image(B, H, W, dt).cuda()
    dense = hip_interp(x, size)
    frame = x.flip(1).permute(0, 2, 3, 1).contiguous()  # [B, H, W, 3] holding B, G, R
    got = torch.empty_like(dense)
    raw(frame.data_ptr() + 2 * frame.element_size(), (H * W * 3, -1, W * 3, 3), got.data_ptr(), got.stride(), ELEM[dt], B, H, W, size)
    assert torch.equal(got, dense)
    # and on the output side: an RGB image stored into a BGR frame
    out_frame = torch.zeros((B,) + size + (3,), device="cuda").to(x.dtype)
    raw(x.data_ptr(), x.stride(), out_frame.data_ptr() + 2 * out_frame.element_size(), (size[0] * size[1] * 3, -1, size[1] * 3, 3), ELEM[dt], B,
        H, W, size)
    assert torch.equal(out_frame.permute(0, 3, 1, 2).flip(1), dense)


@pytest.mark.parametrize("mode", sorted(MODE))
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_the_element_path_gives_the_bits_of_the_16_byte_path(dt, mode):
    """A dense output whose rows are 16-byte aligned takes 16-byte stores; the same dense view one element further on is stored element by
    element.  The width is a multiple of 16 elements, so every row of the first is aligned."""
    B, (H, W), size = 2, (12, 20), (48, 80)
    x = gate_image(B, ((H, W), size), dt).cuda()
    n = B * 3 * size[0] * size[1]
    flat = torch.zeros(n + 16, dtype=x.dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    aligned = hip_interp(x, size, mode=mode, out=flat[:n].view(B, 3, *size)).clone()
    flat.zero_()
    shifted = hip_interp(x, size, mode=mode, out=flat[1:n + 1].view(B, 3, *size))
    assert shifted.data_ptr() % 16 == shifted.element_size() and torch.equal(bits(shifted), bits(aligned))
    assert not bool(flat[0]) and not bool(flat[n + 1:].any())
    if mode != "nearest":
        assert_within_gate(aligned, checker(B, ((H, W), size), dt, mode), dt, f"12x20to48x80 {dt} {mode}")


WINDOWS = {"inside one tile": (TILE_H + 2, TILE_W + 3, 3, 5), "across tile edges": (TILE_H - 3, TILE_W - 5, TILE_H + 4, 2 * TILE_W + 1),
           "last row and column": (2 * TILE_H, 3 * TILE_W - 2, 1, 1), "last rows and columns": (TILE_H + 1, 2 * TILE_W - 1, TILE_H, TILE_W),
           "aligned columns": (3, 16, TILE_H, TILE_W + 32), "everything": (0, 0, 2 * TILE_H + 1, 3 * TILE_W - 1)}


@pytest.mark.parametrize("dt", ["f32", "bf16", "u8"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_a_window_is_that_part_of_the_whole_result(name, dt):
    y0, x0, h, w = WINDOWS[name]
    for ((hin, win), size), mode in ((RAGGED_UP, "bicubic"), (RAGGED_DOWN, "bilinear"), (RAGGED_UP, "nearest")):
        x = image(2, hin, win, dt).cuda()
        whole = hip_interp(x, size, mode=mode)
        part = hip_interp(x, size, mode=mode, window=(y0, x0, h, w))
        assert part.shape == (2, 3, h, w)
        assert torch.equal(part, whole[:, :, y0:y0 + h, x0:x0 + w]), (name, mode)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_the_separable_and_the_gather_path_give_the_same_bits(mode, dt, monkeypatch):
    """Enlarging calls whose tiles lie over at most kInterpStageRows source rows take the separable path; MZ_INTERP_GATHER sends the same
    call down the gather path."""
    for (hin, win), size in (UP3, RAGGED_UP, ((9, 11), (72, 88)), ((41, 41), (90, 41))):
        assert hin <= size[0] and win <= size[1] and (min(TILE_H, size[0]) * hin) // size[0] + 4 <= STAGE_ROWS
        x = image(2, hin, win, dt).cuda()
        monkeypatch.delenv("MZ_INTERP_GATHER", raising=False)
        separable = hip_interp(x, size, mode=mode)
        monkeypatch.setenv("MZ_INTERP_GATHER", "1")
        gathered = hip_interp(x, size, mode=mode)
        torch.cuda.synchronize()
        monkeypatch.delenv("MZ_INTERP_GATHER")
        assert torch.equal(bits(separable), bits(gathered)), (hin, win, size)


# ---- the model's own skip: independent of torch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1_2x_c16", "g3_4x_c16", "g4_8x_c16"])
def test_the_models_skip_is_this_interpolation(name):
    """With the last sub-pixel convolution's weight set to zero, fp32 upscale(x) is the clamped skip alone -- the bicubic of the image
    head's epilogue, accumulated in float32 (about 1e-6 from the float64 kernel here; printed), inside the f32 gate of 1e-5."""
    case = GoldenCase(name)
    r = case.config["upscale_ratio"]
    weights = case.weights()
    last = max(int(k.split(".")[2]) for k in weights if k.startswith("head.layers."))
    key = f"head.layers.{last}.upscale.conv.weight"
    weights[key] = torch.zeros_like(weights[key])
    m = MewZoom(**case.config)
    m.load_state_dict(weights)
    m = m.to("cuda", torch.float32).eval()
    x = case.image().cuda()
    skip = m.upscale(x)
    got = hip_interp(x, scale_factor=r, clamp=True)
    diff = float((skip.double() - got.double()).abs().max())
    print(f"{name}: the model's clamped skip against interpolate(x{r}, clamp): max-abs {diff:.3e}")
    assert skip.shape == got.shape == (case.B, 3, r * case.H, r * case.W)
    assert diff <= 1e-5
    assert_within_gate(got, want64_of(x, (r * case.H, r * case.W), "bicubic").clamp(0, 1), "f32", f"{name} input x{r}")


def model_of(name: str, dt):
    case = GoldenCase(name)
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    return m.to("cuda", dt).eval(), case.image().to("cuda", dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_upscale_and_bicubic_is_its_two_parts(dt):
    m, x = model_of("g3_4x_c16", DTYPES[dt])
    sr, base = m.upscale_and_bicubic(x)
    assert torch.equal(sr, m.upscale(x)) and torch.equal(base, hip_interp(x, scale_factor=4, mode="bicubic", clamp=True))
    assert base.shape == sr.shape and base.dtype == sr.dtype == x.dtype
    x8 = (x.float() * 255).round().to(torch.uint8)
    sr8, base8 = m.upscale_and_bicubic(x8)
    assert sr8.dtype == base8.dtype == torch.uint8
    assert torch.equal(sr8, m.upscale_uint8(x8)) and torch.equal(base8, hip_interp(x8, scale_factor=4, mode="bicubic", clamp=True))
    v = x.contiguous(memory_format=torch.channels_last)  # any strides
    sr_v, base_v = m.upscale_and_bicubic(v)
    assert torch.equal(sr_v, sr) and torch.equal(base_v, base)


# ---- evaluation with the bicubic baseline ------------------------------------------------------------------------------------------------
KEYS = ["psnr", "ssim", "vif", "bicubic_psnr", "bicubic_ssim", "bicubic_vif"]


def close(a: dict, b: dict, keys) -> None:
    for k in keys:
        print(f"{k}: {a[k]!r} against {b[k]!r}, relative difference {abs(a[k] - b[k]) / abs(b[k]):.2e}")
    for k in keys:
        assert a[k] == pytest.approx(b[k], rel=1e-9), (k, a[k], b[k])


def test_evaluate_with_the_baseline_on_the_device_against_the_torch_backend():
    """Both backends round a float64 bicubic once to float32 (the torch one: F.interpolate on float64 tensors), so they measure the same
    baseline image and differ by their metric arithmetic alone: the 1e-9 of tests/test_metrics_gpu.py."""
    import torch.nn.functional as F

    from ultrazoom_amd.evaluate import bicubic_baseline, evaluate
    from ultrazoom_amd.synth import synth_image

    m, _ = model_of("g3_4x_c16", torch.float32)
    pairs = [(F.avg_pool2d(hr, 4), hr) for hr in (synth_image(2, 96, 160, seed=1).cuda(), synth_image(1, 96, 160, seed=2).cuda())]
    a, b = bicubic_baseline(pairs[0][0], (96, 160), "hip"), bicubic_baseline(pairs[0][0], (96, 160), "torch")
    print("baseline images of the two backends differ in", int((a != b).sum()), "of", a.numel(), "elements")
    hip = evaluate(m, pairs, backend="hip", baseline=True)
    ref = evaluate(m, pairs, backend="torch", baseline=True)
    assert list(hip) == list(ref) == ["psnr", "ssim", "vif", "images"] + KEYS[3:]
    close(hip, ref, KEYS)
    assert hip["images"] == ref["images"] == 3
    assert evaluate(m, pairs, backend="hip") == {k: v for k, v in hip.items() if not k.startswith("bicubic_")}
    assert hip["bicubic_psnr"] != hip["psnr"]


def test_evaluate_hr_with_the_baseline_and_a_degradation():
    from ultrazoom_amd import Degradation
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr, lr_from_hr
    from ultrazoom_amd.synth import synth_image

    m, _ = model_of("g3_4x_c16", torch.float32)
    hr = [synth_image(2, 97, 130, seed=9).cuda(), synth_image(1, 97, 130, seed=10).cuda()]
    got = evaluate_hr(m, hr, backend="hip", baseline=True)
    pairs = [lr_from_hr(h, 4, backend="hip") for h in hr]
    close(got, evaluate(m, pairs, backend="torch", baseline=True), KEYS)
    assert {k: v for k, v in got.items() if not k.startswith("bicubic_")} == evaluate_hr(m, hr, backend="hip")
    # with degrade=: the baseline enlarges the DEGRADED input; the torch backend measures the same degraded pairs
    deg = Degradation(seed=11)
    with_deg = evaluate_hr(m, hr, backend="hip", degrade=deg, baseline=True)
    pairs, n = [], 0
    for h in hr:
        lr, target, _ = deg.apply(h, 4, index=n)
        pairs.append((lr, target))
        n += h.shape[0]
    close(with_deg, evaluate(m, pairs, backend="torch", baseline=True), KEYS)
    plain = evaluate_hr(m, hr, backend="hip", degrade=deg)
    assert {k: v for k, v in with_deg.items() if not k.startswith("bicubic_")} == plain and "deg_l2" in plain and with_deg["images"] == 3
    assert with_deg["bicubic_psnr"] < got["bicubic_psnr"]  # blur, noise and JPEG cost the baseline, too
