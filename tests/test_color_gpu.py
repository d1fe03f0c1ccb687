"""The luma kernels on the GPU (mz_luma, mz_metrics_luma; ultrazoom_amd/color.py, metrics.py, evaluate.py).

rgb_to_y equals tests/color_ref.py BIT FOR BIT: the header's arithmetic restated in Python (float64, three fused multiply-adds, one
rounding), on inputs that hold values outside [0, 1], -0, subnormals, the largest finite values (no finite float16 input makes Y
overflow: color_ref says why), infinities, a NaN, and the uint8 colours whose exact Y * 255 is k + 1/2.

The luma metrics are held to the float64 functions of ultrazoom_amd/evaluate.py on the color_ref plane kept in float64, with the standing
tolerances of tests/test_metrics_gpu.py: 1e-12 relative on the squared-error sum, 1e-9 on SSIM and VIF."""

import math
from functools import lru_cache

import pytest
import torch

import color_ref
from color_ref import CODE, DTYPES, ELEM, SHAPES
from ultrazoom_amd import _ffi
from ultrazoom_amd.evaluate import evaluate, luma_plane, ssim_per_image, vif_per_image
from ultrazoom_amd.synth import synth_image

pytestmark = pytest.mark.gpu

SLOTS = _ffi.MZ_METRIC_SLOTS


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def raw_luma(x_ptr, x_strides, out: torch.Tensor, elem, B, H, W, standard="bt601", clamp=0):
    _ffi.luma(x_ptr, x_strides, out.data_ptr(), out.stride(), elem, B, H, W, CODE[standard], clamp, stream())
    torch.cuda.synchronize()
    return out


# ---- rgb_to_y, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rgb_to_y_is_the_reference_bit_for_bit(dt, shape, B):
    from ultrazoom_amd import rgb_to_y

    H, W = shape
    x = color_ref.image(B, H, W, dt).cuda()
    for standard in ("bt601", "full"):
        for clamp in (0, 1):
            got = rgb_to_y(x, standard, clamp=bool(clamp))
            want = color_ref.expected(B, H, W, dt, standard, clamp)
            assert got.shape == (B, 1, H, W) and got.dtype == DTYPES[dt] and got.is_contiguous()
            bad = ~color_ref.image_exact.same_bits(got, want)
            assert not bool(bad.any()), (standard, clamp, int(bad.sum()), got.cpu()[bad][:4], want[bad][:4])


def test_the_planted_ties_are_stored_as_the_reference_stores_them():
    """Every uint8 colour whose exact Y * 255 is k + 1/2 (194 of "bt601", 16 782 of "full"), as one row each."""
    from ultrazoom_amd import rgb_to_y

    for standard in ("bt601", "full"):
        c = color_ref.u8_ties(standard)
        x = torch.from_numpy(c.T.reshape(1, 3, 1, -1).copy())
        want = color_ref.luma_expected(x, standard, "u8", 0)
        assert torch.equal(rgb_to_y(x.cuda(), standard).cpu(), want), standard


VIEWS = ["channels_last", "bgr", "odd_crop", "every_second_image", "grey_broadcast", "out_window", "out_channel_stride"]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("kind", VIEWS)
def test_views_give_the_bits_of_a_dense_copy(kind, dt):
    B, H, W = 2, 9, 70
    x = color_ref.image(B, H, W, dt, special=False).cuda()
    elem, dtype = ELEM[dt], DTYPES[dt]
    dense = raw_luma(x.data_ptr(), x.stride(), torch.empty((B, 1, H, W), dtype=dtype, device="cuda"), elem, B, H, W, clamp=1)
    assert color_ref.same_bits(dense, color_ref.luma_expected(x.cpu(), "bt601", dt, 1))
    out = torch.empty((B, 1, H, W), dtype=dtype, device="cuda")
    if kind == "channels_last":
        v = x.contiguous(memory_format=torch.channels_last)
        assert v.stride() == (3 * H * W, 1, 3 * W, 3)
        got = raw_luma(v.data_ptr(), v.stride(), out, elem, B, H, W, clamp=1)
    elif kind == "bgr":
        frame = x.flip(1).contiguous()  # planes B, G, R: a negative channel stride from the last plane
        got = raw_luma(frame.data_ptr() + 2 * H * W * frame.element_size(), (3 * H * W, -H * W, W, 1), out, elem, B, H, W, clamp=1)
    elif kind == "odd_crop":
        big = torch.zeros((B, 3, H + 4, W + 7), device="cuda", dtype=dtype)
        big[:, :, 1:1 + H, 3:3 + W] = x
        v = big[:, :, 1:1 + H, 3:3 + W]  # rows begin 3 elements into a row of 77: unaligned, the element path
        got = raw_luma(v.data_ptr(), v.stride(), out, elem, B, H, W, clamp=1)
    elif kind == "every_second_image":
        big = torch.zeros((2 * B, 3, H, W), device="cuda", dtype=dtype)
        big[::2] = x
        got = raw_luma(big[::2].data_ptr(), big[::2].stride(), out, elem, B, H, W, clamp=1)
    elif kind == "grey_broadcast":
        grey = x[:, 0:1].contiguous()
        v = grey.expand(B, 3, H, W)
        assert v.stride()[1] == 0
        got = raw_luma(v.data_ptr(), v.stride(), out, elem, B, H, W, clamp=1)
        copy = v.contiguous()
        dense = raw_luma(copy.data_ptr(), copy.stride(), torch.empty_like(out), elem, B, H, W, clamp=1)
    elif kind == "out_window":
        plane = torch.full((B, 1, H + 5, W + 6), 3, device="cuda", dtype=dtype)
        keep = plane.clone()
        win = plane[:, :, 2:2 + H, 5:5 + W]
        got = raw_luma(x.data_ptr(), x.stride(), win, elem, B, H, W, clamp=1)
        keep[:, :, 2:2 + H, 5:5 + W] = dense
        assert torch.equal(plane.view(torch.uint8), keep.view(torch.uint8))  # nothing beside the window is written
    else:  # the output's channel stride names nothing: any value, 0 included
        for cs in (0, -12345, 1):
            out.fill_(3)
            _ffi.luma(x.data_ptr(), x.stride(), out.data_ptr(), (H * W, cs, W, 1), elem, B, H, W, 0, 1, stream())
            torch.cuda.synchronize()
            assert color_ref.same_bits(out, dense), cs
        got = out
    assert color_ref.same_bits(got, dense), kind


def test_rgb_to_y_out_and_refusals_leave_the_library_usable():
    from ultrazoom_amd import rgb_to_y

    x = color_ref.image(2, 5, 64, "bf16").cuda()
    out = torch.empty((2, 1, 5, 64), dtype=torch.bfloat16, device="cuda")
    assert rgb_to_y(x, "full", out=out) is out and color_ref.same_bits(out, color_ref.expected(2, 5, 64, "bf16", "full", 0))
    with pytest.raises(ValueError, match="one shape"):
        rgb_to_y(x, out=torch.empty((2, 3, 5, 64), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(TypeError, match="same dtype"):
        rgb_to_y(x, out=out.float())
    with pytest.raises(_ffi.MewZoomHipError, match="overlap"):
        rgb_to_y(x, out=x[:, 1:2])
    assert color_ref.same_bits(rgb_to_y(x, "full"), color_ref.expected(2, 5, 64, "bf16", "full", 0))


# ---- luma metrics ------------------------------------------------------------------------------------------------------------------------
def rounded(x: torch.Tensor, dt: str) -> torch.Tensor:
    return (x * 255.0).round().to(torch.uint8) if dt == "u8" else x.to(DTYPES[dt])


@lru_cache(maxsize=None)
def pair(B: int, H: int, W: int, dt: str = "f32", seed: int = 31):
    """(pred, target) of the element type on the CPU: a smooth target, image i scaled by 1, 1/2, 1/4, and pred = clamp(target + 0.3
    (noise - 0.5))"""
    scale = torch.tensor([1.0, 0.5, 0.25][:B]).reshape(B, 1, 1, 1)
    target = rounded(synth_image(B, H, W, seed=seed) * scale, dt)
    t = color_ref.values(target)
    pred = rounded((torch.from_numpy(t).float() + 0.3 * (synth_image(B, H, W, seed=seed + 1) - 0.5)).clamp(0, 1), dt)
    return pred, target


@lru_cache(maxsize=None)
def reference(B: int, H: int, W: int, dt: str, standard: str, data_range, shave: int = 0, seed: int = 31):
    """The checker, once per case: evaluate.py's float64 functions on the float64 plane of color_ref"""
    p, t = (torch.from_numpy(color_ref.luma_f64(v[..., shave:H - shave, shave:W - shave].contiguous(), standard)) for v in pair(B, H, W, dt, seed))
    h, w = p.shape[-2:]
    want = {"sq_err": ((p - t) ** 2).sum(dim=(1, 2, 3)), "numel": float(h * w)}
    if min(h, w) >= 11:
        want["ssim"] = ssim_per_image(p, t, data_range)
    if min(h, w) >= 41:
        want["vif"] = vif_per_image(p, t)
    return want


def assert_close(got: torch.Tensor, want: torch.Tensor, rel: float, what: str):
    got, want = got.cpu().tolist(), want.tolist()
    print(f"{what}: got {got} want {want}")
    for g, w in zip(got, want):
        assert math.isclose(g, w, rel_tol=rel), (what, g, w, abs(g - w) / max(abs(w), 1e-300))


def check_metrics(B, H, W, dt, standard, data_range, shave=0):
    from ultrazoom_amd.metrics import image_metrics

    p, t = (v.cuda() for v in pair(B, H, W, dt))
    want = reference(B, H, W, dt, standard, data_range, shave)
    which = tuple(k for k in ("psnr", "ssim", "vif") if k in want or k == "psnr")
    got = image_metrics(p, t, which=which, data_range=data_range, luma=standard, shave=shave)
    assert_close(got["sq_err"], want["sq_err"], 1e-12, "sq_err")
    assert got["numel"].cpu().tolist() == [want["numel"]] * B
    for k in which[1:]:
        assert got[k].shape == (B,)
        assert_close(got[k], want[k], 1e-9, k)


# 11 x 11: one window; 26 x 42 and 27 x 43: one 16 x 32 tile of the valid map and one pixel past it; 41 x 41: the VIF minimum
@pytest.mark.parametrize("data_range", [None, 1.0])
@pytest.mark.parametrize("B, shape", [(1, (11, 11)), (1, (26, 42)), (2, (27, 43)), (1, (41, 41)), (3, (75, 93))], ids=lambda v: str(v).replace(" ", ""))
def test_luma_metrics_at_the_sizes_where_the_kernels_can_go_wrong(B, shape, data_range):
    for standard in ("bt601", "full"):
        check_metrics(B, *shape, "f32", standard, data_range)


@pytest.mark.parametrize("shave", [0, 4])
@pytest.mark.parametrize("data_range", [None, 1.0])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_luma_metrics_of_every_element_type_shaved_and_whole(dt, data_range, shave):
    check_metrics(2, 49, 51, dt, "bt601", data_range, shave)  # (49 x 51 shaved by 4 is 41 x 43: VIF still runs)


def raw_metrics(p: torch.Tensor, t: torch.Tensor, which=7, data_range=-1.0, standard=0, fill=0.0):
    B, _, H, W = p.shape
    need = _ffi.metrics_luma_workspace_bytes(B, H, W, which)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((B, SLOTS), fill, dtype=torch.float64, device="cuda")
    _ffi.metrics_luma(p.data_ptr(), p.stride(), t.data_ptr(), t.stride(), _ffi.elem_code(p.dtype), B, H, W, which, standard, data_range, 2.0,
                      out.data_ptr(), ws.data_ptr(), need, stream())
    torch.cuda.synchronize()
    return out


def test_two_calls_give_the_same_bits_and_images_do_not_depend_on_their_batch():
    p, t = (v.cuda() for v in pair(3, 59, 77, "bf16"))
    first, second = raw_metrics(p, t), raw_metrics(p, t)
    assert torch.equal(first, second) and not bool(first[:, [0, 6, 8, 11]].isnan().any())
    fixed = raw_metrics(p, t, data_range=1.0)
    for i in range(3):
        alone = raw_metrics(p[i:i + 1], t[i:i + 1], data_range=1.0)
        assert torch.equal(alone[0], fixed[i]), (i, alone[0], fixed[i])
    # data_range <= 0 is the range of the Y planes of the BATCH
    yp, yt = (torch.from_numpy(color_ref.luma_f64(v.cpu(), "bt601")) for v in (p, t))
    assert first[:, 14].cpu().tolist() == [float(max(yp.max() - yp.min(), yt.max() - yt.min()))] * 3
    assert first[:, 2].cpu().tolist() == yp.amin(dim=(1, 2, 3)).tolist() and first[:, 5].cpu().tolist() == yt.amax(dim=(1, 2, 3)).tolist()


@pytest.mark.parametrize("which", [7, 1, 2, 4, 6])
def test_the_slots_that_are_not_the_calls_to_write_keep_a_planted_pattern(which):
    p, t = (v.cuda() for v in pair(2, 45, 52, "f16"))
    full = raw_metrics(p, t, which=which, data_range=1.0)
    got = raw_metrics(p, t, which=which, data_range=1.0, fill=-123.25)
    written = sorted(set(([0, 1, 2, 3, 4, 5] if which & 1 else []) + ([6, 7, 14] if which & 2 else []) + ([8, 11] if which & 4 else [])))
    kept = [s for s in range(SLOTS) if s not in written]
    assert {9, 10, 12, 13, 15} <= set(kept)
    assert torch.equal(got[:, written], full[:, written]) and not bool(got[:, written].isnan().any())
    assert bool((got[:, kept] == -123.25).all()), f"slots {kept} are not {which}'s to write: {got}"
    if which & 1:
        assert got[:, 1].tolist() == [45.0 * 52.0] * 2  # one plane's elements
    if which & 2:
        assert got[:, 7].tolist() == [35.0 * 42.0] * 2
    # SSIM with the batch's range takes it from the PSNR pass: slots 0..5 are written then, too
    if which == 2:
        batch = raw_metrics(p, t, which=2, data_range=-1.0, fill=-123.25)
        assert bool((batch[:, [8, 9, 10, 11, 12, 13, 15]] == -123.25).all()) and bool((batch[:, :8] != -123.25).all())


def test_views_of_the_pair_give_the_bits_of_dense_copies():
    B, H, W = 2, 45, 52
    p, t = (v.cuda() for v in pair(B, H, W, "u8"))
    dense = raw_metrics(p, t)
    pc = p.contiguous(memory_format=torch.channels_last)
    big = torch.zeros((B, 3, H + 3, W + 5), dtype=torch.uint8, device="cuda")
    big[:, :, 2:2 + H, 1:1 + W] = t
    assert torch.equal(raw_metrics(pc, big[:, :, 2:2 + H, 1:1 + W]), dense)
    # MATLAB's rounded-Y variant: the uint8 Y planes broadcast to three equal channels through the RGB entry
    from ultrazoom_amd import rgb_to_y
    from ultrazoom_amd.metrics import image_metrics

    yp, yt = rgb_to_y(p), rgb_to_y(t)
    got = image_metrics(yp.expand(-1, 3, -1, -1), yt.expand(-1, 3, -1, -1), which=("psnr",))
    d = yp.cpu().double() / 255 - yt.cpu().double() / 255
    assert_close(got["sq_err"], 3 * (d * d).sum(dim=(1, 2, 3)), 1e-12, "sq_err of the rounded Y planes")


def test_accumulator_with_luma_and_shave_matches_the_classes_of_evaluate():
    from ultrazoom_amd.evaluate import PSNR, SSIM, VIF
    from ultrazoom_amd.metrics import MetricsAccumulator

    acc = MetricsAccumulator(luma="bt601", shave=4)
    psnr, ssim, vif = PSNR(1.0), SSIM(), VIF()
    for B, H, W, dt in [(2, 49, 51, "bf16"), (1, 48, 51, "bf16")]:  # the second leaves 40 rows: no VIF from it
        p, t = pair(B, H, W, dt)
        acc.update(p.cuda(), t.cuda())
        yp, yt = (torch.from_numpy(color_ref.luma_f64(v[..., 4:H - 4, 4:W - 4].contiguous(), "bt601")) for v in (p, t))
        psnr.update(yp, yt)
        ssim.update(yp, yt)
        if H - 8 >= 41:
            vif.update(yp, yt)
    got = acc.compute()
    assert math.isclose(got["psnr"], psnr.compute(), rel_tol=1e-12)
    assert math.isclose(got["ssim"], ssim.compute(), rel_tol=1e-9)
    assert math.isclose(got["vif"], vif.compute(), rel_tol=1e-9) and vif.n == 2


def test_evaluate_hip_backend_with_luma_shave_and_baseline_matches_the_torch_backend():
    """The two backends form Y with and without fma, which moves a luma difference by at most 6 * 2^-54 and sq_err by at most
    2 * 3.4e-16 / rms(d) relative: the pairs must have a luma RMS difference of at least 1e-2, asserted here on the torch side."""
    from golden_util import GoldenCase
    from ultrazoom_amd import MewZoom

    case = GoldenCase("g1_2x_c16")
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    m = m.to("cuda").eval()
    x = synth_image(2, 40, 56, seed=6, smooth=False)  # hash noise in, a smooth target
    y = synth_image(2, 80, 112, seed=7)
    seen = []

    class Copies:  # the torch backend fed with CPU copies of the same upscale results
        def upscale(self, x_cpu):
            up = m.upscale(x_cpu.cuda()).cpu()
            seen.append(up)
            return up

    got = evaluate(m, [(x.cuda(), y.cuda())], backend="hip", luma="bt601", shave=2, baseline=True)
    want = evaluate(Copies(), [(x, y)], backend="torch", luma="bt601", shave=2, baseline=True)
    from ultrazoom_amd.evaluate import bicubic_baseline

    for img in (seen[0], bicubic_baseline(x, (80, 112))):
        d = (luma_plane(img, "bt601") - luma_plane(y, "bt601"))[..., 2:-2, 2:-2]
        rms = float((d * d).mean().sqrt())
        print("luma rms difference", rms)
        assert rms >= 1e-2
    print(got, want)
    assert got["images"] == want["images"] == 2 and set(got) == set(want)
    for key in ("", "bicubic_"):
        assert math.isclose(got[key + "psnr"], want[key + "psnr"], rel_tol=1e-12), key
        assert math.isclose(got[key + "ssim"], want[key + "ssim"], rel_tol=1e-9), key
        assert math.isclose(got[key + "vif"], want[key + "vif"], rel_tol=1e-9), key
