"""The degradation kernels (mz_blur, mz_noise, mz_jpeg; ultrazoom_amd/degrade.py) against the CPU checkers of tests/degrade_ref.py.

Shapes put the edges where they can go wrong: 16x16 (one MCU, half a blur tile), 17x33 and 31x15 (H, W = 1 and 15 mod 16, a second blur
tile column), 37x45, 64x80 (several tiles of every kernel, W = 0 mod 16).  Inputs are uniform noise rounded to the element type first.

Gates:
  blur   those of tests/test_resize_gpu.py::assert_within_gate (float64 accumulation, float32 between the passes)
  noise  one ulp of the storage type at the checker's float64 value; uint8: at most 1 LSB, on at most 0.1 % of the elements (both sides
         evaluate ln and cos in float64, from different libraries; tests/test_degrade_cpu.py shows fewer than 0.1 % of the checker's own
         values lie within 1e-6 of a rounding tie)
  JPEG   bit for bit outside the pixels fed by a near-tie block (a coefficient with c / Q within 1e-6 of a half); those blocks are under
         1 % per case (tests/test_degrade_cpu.py; expected about 1e-4).  Against the codec fixture: mean-abs <= 1.05 x the checker's own
         recorded distance (tests/golden/degrade_codec.json).
Everything else is an equality."""

import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import degrade_ref as R
from degrade_ref import BATCH, BLUR_SIGMAS, DTYPES, ELEM, NOISE_SIGMAS, OFFSET, QUALITIES, SEED, SHAPES, hip, image, shape_id
from gpu_util import ulp_of
from resize_util import assert_within_gate, model_and_input
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- blur --------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def blur_checker(B, shape, dt, sigma):
    return R.blur_ref(image(B, *shape, dt), sigma)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_blur_against_the_float64_checker(shape, dt):
    x = image(BATCH, *shape, dt)
    xg = x.cuda()
    for sigma in BLUR_SIGMAS:
        if int(3 * sigma) >= min(shape):
            continue
        got = hip().gaussian_blur(xg, sigma)
        assert_within_gate(got, blur_checker(BATCH, shape, dt, sigma), dt, f"blur {shape_id(shape)} {dt} sigma {sigma}")
        if sigma == 0.2:
            assert torch.equal(got.cpu(), x), "sigma < 1 / 3 copies"
    # per-image sigmas: one call per image, each equal to that image of the scalar call
    per = hip().gaussian_blur(xg, [0.34, 1.0, 0.2])
    for b, s in enumerate((0.34, 1.0, 0.2)):
        assert torch.equal(per[b], hip().gaussian_blur(xg, s)[b]), b


def raw_blur(x_ptr, x_strides, out, elem, B, H, W, sigma):
    _ffi.blur(x_ptr, x_strides, out.data_ptr(), out.stride(), elem, B, H, W, sigma, stream())
    torch.cuda.synchronize()
    return out


def views_of(x: torch.Tensor, dt: str):
    """name -> a non-contiguous view equal to x"""
    B, _, H, W = x.shape
    big = torch.full((B, 3, H + 7, W + 9), float("nan") if dt != "u8" else 255, device="cuda").to(x.dtype)
    big[:, :, 3:3 + H, 5:5 + W] = x
    return {"channels_last": x.contiguous(memory_format=torch.channels_last), "hwc_frame": x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2),
            "crop": big[:, :, 3:3 + H, 5:5 + W]}


@pytest.mark.parametrize("dt", ["bf16", "u8", "f32"])
def test_views_give_the_bits_of_a_dense_copy(dt):
    B, (H, W) = 2, (37, 45)
    x = image(B, H, W, dt).cuda()
    dense = {"blur": hip().gaussian_blur(x, 1.0), "noise": hip().gaussian_noise(x, 0.1, seed=SEED, offset=OFFSET), "jpeg": hip().jpeg(x, 50)}
    for kind, v in views_of(x, dt).items():
        assert not v.is_contiguous() and torch.equal(v, x)
        assert torch.equal(hip().gaussian_blur(v, 1.0), dense["blur"]), kind
        assert torch.equal(hip().gaussian_noise(v, 0.1, seed=SEED, offset=OFFSET), dense["noise"]), kind
        assert torch.equal(hip().jpeg(v, 50), dense["jpeg"]), kind
    # BGR through a negative channel stride
    frame = x.flip(1).permute(0, 2, 3, 1).contiguous()  # [B, H, W, 3] holding B, G, R
    ptr, strides = frame.data_ptr() + 2 * frame.element_size(), (H * W * 3, -1, W * 3, 3)
    assert torch.equal(raw_blur(ptr, strides, torch.empty_like(x), ELEM[dt], B, H, W, 1.0), dense["blur"])
    out = torch.empty_like(x)
    _ffi.noise(ptr, strides, out.data_ptr(), out.stride(), ELEM[dt], B, H, W, 0.1, SEED, OFFSET, stream())
    assert torch.equal(out, dense["noise"])
    need = _ffi.jpeg_workspace_bytes(B, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(x)
    _ffi.jpeg(ptr, strides, out.data_ptr(), out.stride(), ELEM[dt], B, H, W, 50, ws.data_ptr(), need, stream())
    assert torch.equal(out, dense["jpeg"])


def test_a_blur_wider_than_the_image_is_refused():
    x = image(1, 37, 45, "f32").cuda()
    small = x[:, :, :5, :5].contiguous()
    with pytest.raises(ValueError, match="reflect"):
        hip().gaussian_blur(small, 1.7)
    with pytest.raises(_ffi.MewZoomHipError, match="reflect"):
        raw_blur(small.data_ptr(), small.stride(), torch.empty_like(small), 0, 1, 5, 5, 1.7)
    with pytest.raises(_ffi.MewZoomHipError, match="overlap"):
        raw_blur(x.data_ptr(), x.stride(), x, 0, 1, 37, 45, 1.0)
    assert_within_gate(hip().gaussian_blur(small, 1.6), R.blur_ref(small, 1.6), "f32", "5x5 sigma 1.6 (half 4), after the refusals")


# ---- noise -------------------------------------------------------------------------------------------------------------------------------
def assert_noise_gate(got: torch.Tensor, want64: torch.Tensor, dt: str, what: str) -> None:
    got = got.cpu()
    assert got.dtype == DTYPES[dt] and got.shape == want64.shape
    if dt == "u8":
        want = torch.floor(want64 * 255 + 0.5)
        diff = (got.double() - want).abs()
        share = float((diff != 0).double().mean())
        print(f"{what}: {int((diff != 0).sum())} of {diff.numel()} elements differ (max {float(diff.max())})")
        assert float(diff.max()) <= 1 and share <= 1e-3, (what, float(diff.max()), share)
        return
    diff = (got.double() - want64).abs()
    if dt == "f32":
        _, e = torch.frexp(want64.float().abs())
        ulp = torch.ldexp(torch.ones_like(want64), (e - 1).clamp(min=-126) - 23)  # float32's spacing at |want64|
    else:
        ulp = ulp_of(want64, dt).double()
    excess = float((diff / ulp).max())
    print(f"{what}: max-abs {float(diff.max()):.3e}, {excess:.3f} ulp")
    assert excess <= 1.0, (what, excess)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_noise_against_the_checker(shape, dt):
    x = image(BATCH, *shape, dt)
    xg = x.cuda()
    for sigma in NOISE_SIGMAS:
        got = hip().gaussian_noise(xg, sigma, seed=SEED, offset=OFFSET)
        assert_noise_gate(got, R.noise_ref(x, sigma, SEED, OFFSET), dt, f"noise {shape_id(shape)} {dt} sigma {sigma}")
    whole = hip().gaussian_noise(xg, 0.05, seed=SEED, offset=OFFSET)
    # a batched call equals per-image calls with offset + b, through the C entry and through a sequence of sigmas
    for b in range(BATCH):
        assert torch.equal(hip().gaussian_noise(xg[b:b + 1], 0.05, seed=SEED, offset=OFFSET + b)[0], whole[b]), b
    assert torch.equal(hip().gaussian_noise(xg, [0.05] * BATCH, seed=SEED, offset=OFFSET), whole)
    # in place equals out of place
    y = xg.clone()
    assert hip().gaussian_noise(y, 0.05, seed=SEED, offset=OFFSET, out=y).data_ptr() == y.data_ptr() and torch.equal(y, whole)
    # another seed, another stream: other bits
    assert not torch.equal(hip().gaussian_noise(xg, 0.05, seed=SEED + 1, offset=OFFSET), whole)
    assert not torch.equal(hip().gaussian_noise(xg, 0.05, seed=SEED, offset=OFFSET + 1), whole)
    # sigma = 0 gives the clamped input
    if dt == "u8":
        assert torch.equal(hip().gaussian_noise(xg, 0.0, seed=SEED), xg)
    else:
        wide = (xg.float() * 1.5 - 0.25).to(xg.dtype)
        assert torch.equal(hip().gaussian_noise(wide, 0.0, seed=SEED), wide.clamp(0, 1))


# ---- JPEG --------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def jpeg_checker(B, shape, dt, q):
    return R.jpeg_expected(image(B, *shape, dt), q, DTYPES[dt])


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_jpeg_is_the_checker_bit_for_bit(shape, dt):
    xg = image(BATCH, *shape, dt).cuda()
    for q in QUALITIES:
        want, unsure, share = jpeg_checker(BATCH, shape, dt, q)
        got = hip().jpeg(xg, q).cpu()
        assert got.dtype == want.dtype and got.shape == want.shape
        keep = ~unsure.expand_as(want)
        wrong = int(((got != want) & keep).sum())
        print(f"jpeg {shape_id(shape)} {dt} q {q}: {wrong} elements differ outside near-tie blocks; near-tie share {share:.2e}, "
              f"{int(((got != want) & ~keep).sum())} differ inside")
        assert share < 0.01, (q, share)
        assert wrong == 0, (q, wrong)
    # per-image qualities
    per = hip().jpeg(xg, [20, 90, 50])
    for b, q in enumerate((20, 90, 50)):
        assert torch.equal(per[b], hip().jpeg(xg, q)[b]), b


def test_jpeg_against_the_codec_fixture():
    codec = np.load(GOLDEN / "d1_jpeg_codec.npz")
    record = json.loads((GOLDEN / "degrade_codec.json").read_text())
    for i in range(3):
        x = torch.from_numpy(codec[f"in_{i}"])[None].cuda()
        for q in QUALITIES:
            got = hip().jpeg(x, q)[0].cpu().numpy().astype(np.int64)
            mean_abs = float(np.abs(got - codec[f"out_{i}_q{q}"].astype(np.int64)).mean())
            print(f"image {i} q {q}: GPU mean-abs {mean_abs:.4f}, checker {record[f'{i}_q{q}']['mean_abs']:.4f}")
            assert mean_abs <= 1.05 * record[f"{i}_q{q}"]["mean_abs"], (i, q, mean_abs)


@pytest.mark.parametrize("dt", ["u8", "bf16"])
def test_jpeg_constant_image_nan_workspace_and_output_views(dt):
    B, (H, W) = 2, (37, 45)
    # a constant image stays constant at q = 100
    for v in (0, 77, 255):
        c = torch.full((1, 3, 17, 33), v, dtype=torch.uint8)
        c = c.cuda() if dt == "u8" else (c.float() / 255).to(DTYPES[dt]).cuda()
        assert torch.equal(hip().jpeg(c, 100), c), v
    # a NaN-filled workspace gives the same bits
    x = image(B, H, W, dt).cuda()
    want = hip().jpeg(x, 50)
    need = _ffi.jpeg_workspace_bytes(B, H, W)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    got = torch.empty_like(want)
    _ffi.jpeg(x.data_ptr(), x.stride(), got.data_ptr(), got.stride(), ELEM[dt], B, H, W, 50, ws.data_ptr(), need, stream())
    assert torch.equal(got, want)
    # output views are written in place, and nothing else
    mark = 77 if dt == "u8" else 0.4375
    for kind in ("hwc_frame", "crop_of_a_canvas", "every_second_image"):
        shape = {"hwc_frame": (B, H, W, 3), "crop_of_a_canvas": (B, 3, H + 6, W + 10), "every_second_image": (2 * B, 3, H, W)}[kind]
        canvas = torch.full(shape, mark, device="cuda").to(x.dtype)
        view_of = {"hwc_frame": lambda t: t.permute(0, 3, 1, 2), "crop_of_a_canvas": lambda t: t[:, :, 2:2 + H, 7:7 + W],
                   "every_second_image": lambda t: t[1::2]}[kind]
        expect = canvas.clone()
        view_of(expect).copy_(want)
        out = view_of(canvas)
        assert hip().jpeg(x, 50, out=out).data_ptr() == out.data_ptr()
        assert torch.equal(canvas, expect), kind
        for fn, ref in ((lambda o: hip().gaussian_blur(x, 1.0, out=o), hip().gaussian_blur(x, 1.0)),
                        (lambda o: hip().gaussian_noise(x, 0.1, seed=SEED, out=o), hip().gaussian_noise(x, 0.1, seed=SEED))):
            canvas.fill_(mark)
            expect = canvas.clone()
            view_of(expect).copy_(ref)
            fn(view_of(canvas))
            assert torch.equal(canvas, expect), kind


# ---- Degradation and evaluate_hr ---------------------------------------------------------------------------------------------------------
def test_degradation_apply():
    from ultrazoom_amd import Degradation
    from ultrazoom_amd.synth import synth_image

    deg = Degradation(seed=3)
    hr = synth_image(3, 50, 67, seed=9).to("cuda", torch.bfloat16)
    lr, cropped, targets = deg.apply(hr, 4, index=7)
    assert lr.shape == (3, 3, 12, 16) and lr.dtype == hr.dtype and cropped.shape == (3, 3, 48, 64) and cropped.data_ptr() == hr.data_ptr()
    params = deg.sample(3, 7)
    assert targets.shape == (3, 3) and targets.dtype == torch.float32 and targets.is_cuda
    assert torch.equal(targets.cpu(), torch.tensor(deg.targets(params), dtype=torch.float32))
    assert float(targets.min()) >= 0.0 and float(targets.max()) <= 1.0
    # the chain, step by step
    from ultrazoom_amd.resize import resize

    x = hip().gaussian_blur(cropped, [p[0] for p in params])
    x = hip().gaussian_noise(x, [p[1] for p in params], seed=3, offset=7)
    x = hip().jpeg(resize(x, (12, 16)), [int(100 * (1 - p[2])) for p in params])
    assert torch.equal(lr, x)
    # determinism from the seed and the index; an image does not depend on its batch
    again = deg.apply(hr, 4, index=7)
    assert torch.equal(again[0], lr) and torch.equal(again[2], targets)
    assert torch.equal(deg.apply(hr[1:2], 4, index=8)[0][0], lr[1])
    assert not torch.equal(Degradation(seed=4).apply(hr, 4, index=7)[0], lr)
    assert torch.equal(hr, synth_image(3, 50, 67, seed=9).to("cuda", torch.bfloat16)), "the input is not written"


def test_evaluate_hr_with_a_degradation():
    from ultrazoom_amd import Degradation
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr, lr_from_hr
    from ultrazoom_amd.synth import synth_image

    m, _ = model_and_input("bf16")
    deg = Degradation(seed=0)
    batches = [synth_image(2, 176, 180, seed=9).to("cuda", torch.bfloat16), synth_image(1, 176, 180, seed=10).to("cuda", torch.bfloat16)]
    got = evaluate_hr(m, batches, backend="hip", degrade=deg)
    print(got)
    assert set(got) == {"psnr", "ssim", "vif", "deg_l2", "images"} and got["images"] == 3 and got["vif"] is not None
    pairs, sq, count, n = [], 0.0, 0, 0
    for hr in batches:
        lr, target, want = deg.apply(hr, m.upscale_ratio, index=n)
        pairs.append((lr, target))
        qa = m.forward(lr)[1]
        sq += float(((qa.double().cpu() - want.double().cpu()) ** 2).sum())
        count += qa.numel()
        n += hr.shape[0]
    assert abs(got["deg_l2"] - sq / count) <= 1e-12 * max(1.0, sq / count)
    want = evaluate(m, pairs, backend="hip")
    assert {k: got[k] for k in want} == want
    # without degrade: today's result
    assert evaluate_hr(m, batches, backend="hip") == evaluate(m, [lr_from_hr(hr, m.upscale_ratio, backend="hip") for hr in batches], backend="hip")
    with pytest.raises(ValueError, match="backend='hip'"):
        evaluate_hr(m, batches, degrade=deg)


# ---- the lower edge ----------------------------------------------------------------------------------------------------------------------
# One pixel, a single row, a single column, 2 x 3, one whole MCU and 9 x 15 (partial MCUs in both directions).  A list of its own: SHAPES
# is shared with sigma 2.5, whose reflection needs eight pixels.
SMALL_SHAPES = [(1, 1), (1, 9), (7, 1), (2, 3), (8, 8), (9, 15)]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=shape_id)
def test_noise_at_the_smallest_images(shape, dt):
    x = image(BATCH, *shape, dt)
    xg = x.cuda()
    for sigma in NOISE_SIGMAS:
        got = hip().gaussian_noise(xg, sigma, seed=SEED, offset=OFFSET)
        assert_noise_gate(got, R.noise_ref(x, sigma, SEED, OFFSET), dt, f"noise {shape_id(shape)} {dt} sigma {sigma}")
    whole = hip().gaussian_noise(xg, 0.05, seed=SEED, offset=OFFSET)
    for b in range(BATCH):
        assert torch.equal(hip().gaussian_noise(xg[b:b + 1], 0.05, seed=SEED, offset=OFFSET + b)[0], whole[b]), b


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=shape_id)
def test_jpeg_at_the_smallest_images_is_the_checker_bit_for_bit(shape, dt):
    xg = image(BATCH, *shape, dt).cuda()
    for q in QUALITIES:
        want, unsure, share = jpeg_checker(BATCH, shape, dt, q)
        got = hip().jpeg(xg, q).cpu()
        assert got.dtype == want.dtype and got.shape == want.shape
        keep = ~unsure.expand_as(want)
        wrong = int(((got != want) & keep).sum())
        print(f"jpeg {shape_id(shape)} {dt} q {q}: {wrong} elements differ outside near-tie blocks; near-tie share {share:.2e}")
        assert share < 0.01, (q, share)
        assert wrong == 0, (q, wrong)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=shape_id)
def test_blur_at_the_smallest_images(shape, dt):
    """Every sigma whose reflection fits (int(3 sigma) < min(H, W)) against the checker; every other one is refused with its message, by
    the Python layer and by the C entry, and the call after a refusal is unaffected."""
    x = image(BATCH, *shape, dt)
    xg = x.cuda()
    refused = 0
    for sigma in BLUR_SIGMAS:
        if int(3 * sigma) < min(shape):
            got = hip().gaussian_blur(xg, sigma)
            assert_within_gate(got, R.blur_ref(x, sigma), dt, f"blur {shape_id(shape)} {dt} sigma {sigma}")
            continue
        refused += 1
        with pytest.raises(ValueError, match="reflect"):
            hip().gaussian_blur(xg, sigma)
        out = torch.empty_like(xg)
        with pytest.raises(_ffi.MewZoomHipError, match="reflect"):
            raw_blur(xg.data_ptr(), xg.stride(), out, ELEM[dt], BATCH, *shape, sigma)
        assert torch.equal(hip().gaussian_blur(xg, 0.2).cpu(), x), "the call after a refusal"
    assert refused == sum(int(3 * s) >= min(shape) for s in BLUR_SIGMAS) and (refused > 0) == (min(shape) < 8)
    assert torch.equal(hip().gaussian_blur(xg, 0.2).cpu(), x), "sigma < 1 / 3 copies"
