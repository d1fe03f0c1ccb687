"""The metrics kernels (mz_metrics, ultrazoom_amd/metrics.py) against the float64 functions of ultrazoom_amd/evaluate.py run on CPU tensors
(tests/test_evaluate.py pins those to numpy / scipy).  Inputs are rounded to the element type first, so both sides see the same values.

Tolerances: 1e-9 relative for SSIM and VIF per image (what tests/test_evaluate.py allows between its two float64 computations of the
same quantities; with c2 >= 8.1e-4 the float64 rounding of a windowed moment, <= 121 * 2^-53, stays orders below it), 1e-12 relative for
the squared-error sum (<= 3 * 57 * 105 float64 additions of exact terms in another order), an exact element count."""

import math
import re
from functools import lru_cache
from pathlib import Path

import pytest
import torch

from ultrazoom_amd import _ffi
from ultrazoom_amd.evaluate import PSNR, SSIM, VIF, evaluate, ssim_per_image, vif_per_image
from ultrazoom_amd.synth import synth_image

pytestmark = pytest.mark.gpu

HEADER = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_metrics.h").read_text()
TILE_H = int(re.search(r"constexpr int kMetricsTileH = (\d+);", HEADER).group(1))
TILE_W = int(re.search(r"constexpr int kMetricsTileW = (\d+);", HEADER).group(1))
# the SSIM map of an H x W image is (H - 10) x (W - 10): one pixel more than two tiles, one pixel less than three, in both directions
SSIM_SHAPES = [(11, 11), (12, 13), (2 * TILE_H + 1 + 10, 2 * TILE_W + 1 + 10), (3 * TILE_H - 1 + 10, 3 * TILE_W - 1 + 10)]
VIF_SHAPES = [(41, 41), (42, 57), (64, 80)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.uint8}
SCALES = (1.0, 0.5, 0.25)  # image i of a batch spans [0, SCALES[i]]: a per-image data range differs from the batch's


def rounded(x: torch.Tensor, dt: str) -> torch.Tensor:
    """float32 CPU values in [0, 1] -> the element type"""
    return (x * 255.0).round().to(torch.uint8) if dt == "u8" else x.to(DTYPES[dt])


def as_double(x: torch.Tensor) -> torch.Tensor:
    x = x.cpu()
    return x.double() / 255 if x.dtype == torch.uint8 else x.double()


@lru_cache(maxsize=None)
def pair(B: int, H: int, W: int, a: float, dt: str = "f32", seed: int = 11):
    """(pred, target) of the element type, on the CPU: pred = clamp(target + a (synth - 0.5))"""
    scale = torch.tensor(SCALES[:B] if B <= 3 else [1.0] * B).reshape(B, 1, 1, 1)
    target = rounded(synth_image(B, H, W, seed=seed) * scale, dt)
    t = as_double(target).float()
    pred = rounded((t + a * (synth_image(B, H, W, seed=seed + 1) - 0.5)).clamp(0, 1), dt)
    return pred, target


@lru_cache(maxsize=None)
def reference(B: int, H: int, W: int, a: float, dt: str, data_range, with_vif: bool, seed: int = 11):
    """The checker, once per case: evaluate.py's float64 functions on CPU tensors"""
    p, t = (as_double(v) for v in pair(B, H, W, a, dt, seed))
    want = {"sq_err": ((p - t) ** 2).sum(dim=(1, 2, 3)), "numel": float(p[0].numel())}
    if min(H, W) >= 11:
        want["ssim"] = ssim_per_image(p, t, data_range)
    if with_vif:
        want["vif"] = vif_per_image(p, t)
    return want


def assert_close(got: torch.Tensor, want: torch.Tensor, rel: float, what: str):
    got, want = got.cpu().tolist(), want.tolist()
    print(f"{what}: got {got} want {want}")
    for g, w in zip(got, want):
        assert math.isclose(g, w, rel_tol=rel), (what, g, w, abs(g - w) / max(abs(w), 1e-300))


def hip_metrics(pred, target, **kw):
    from ultrazoom_amd.metrics import image_metrics

    return image_metrics(pred.cuda(), target.cuda(), **kw)


def raw(pred_ptr, pred_strides, target_ptr, target_strides, elem, B, H, W, which=7, data_range=-1.0):
    """mz_metrics on raw views (negative strides, which torch tensors cannot express): the whole [B, slots] output"""
    need = _ffi.metrics_workspace_bytes(B, H, W, which)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros((B, _ffi.MZ_METRIC_SLOTS), dtype=torch.float64, device="cuda")
    _ffi.metrics(pred_ptr, pred_strides, target_ptr, target_strides, elem, B, H, W, which, data_range, 2.0, out.data_ptr(), ws.data_ptr(),
                 need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def raw_of(pred: torch.Tensor, target: torch.Tensor, **kw):
    elem = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.uint8: 3}[pred.dtype]
    B, _, H, W = pred.shape
    return raw(pred.data_ptr(), pred.stride(), target.data_ptr(), target.stride(), elem, B, H, W, **kw)


@pytest.mark.parametrize("data_range", [None, 1.0])
@pytest.mark.parametrize("a", [0.05, 0.3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_psnr_and_ssim_at_the_tile_edges(shape, B, a, data_range):
    H, W = shape
    p, t = pair(B, H, W, a)
    want = reference(B, H, W, a, "f32", data_range, False)
    got = hip_metrics(p, t, which=("psnr", "ssim"), data_range=data_range)
    assert got["sq_err"].dtype == torch.float64 and got["ssim"].is_cuda and got["ssim"].shape == (B,)
    assert_close(got["sq_err"], want["sq_err"], 1e-12, "sq_err")
    assert got["numel"].cpu().tolist() == [want["numel"]] * B
    assert_close(got["ssim"], want["ssim"], 1e-9, "ssim")


@pytest.mark.parametrize("a", [0.05, 0.3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", VIF_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vif_at_every_decimation(shape, B, a):
    H, W = shape
    p, t = pair(B, H, W, a)
    want = reference(B, H, W, a, "f32", None, True)
    got = hip_metrics(p, t, which=("vif",))
    assert set(got) == {"vif"} and got["vif"].shape == (B,)
    assert_close(got["vif"], want["vif"], 1e-9, "vif")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_every_element_type(dt):
    B, H, W, a = 2, 64, 80, 0.3
    p, t = pair(B, H, W, a, dt)
    assert p.dtype == DTYPES[dt]
    want = reference(B, H, W, a, dt, None, True)
    got = hip_metrics(p, t)
    assert_close(got["sq_err"], want["sq_err"], 1e-12, "sq_err")
    assert got["numel"].cpu().tolist() == [want["numel"]] * B
    assert_close(got["ssim"], want["ssim"], 1e-9, "ssim")
    assert_close(got["vif"], want["vif"], 1e-9, "vif")


def flat_pair():
    t = torch.full((1, 3, 64, 64), 0.5)
    p = t.clone()
    p[..., 32:] = 0.5039
    return p, t


def test_nearly_flat_pair_needs_float64_moments():
    """target 0.5 everywhere, pred 0.5 / 0.5039 in halves, data_range=None: c2 ~ 1.4e-8.  float64 moment rounding of a few 1e-14
    against it moves SSIM by ~1e-6 at most; float32 moments give 0.04 instead of 0.84."""
    p, t = flat_pair()
    want = ssim_per_image(p.double(), t.double(), None)
    got = hip_metrics(p, t, which=("ssim",))["ssim"].cpu()
    print("flat pair: got", got.tolist(), "want", want.tolist())
    assert 0.8 < float(want[0]) < 0.9
    assert abs(float(got[0]) - float(want[0])) <= 1e-5


def test_flat_target_gives_nan_vif_on_both_sides():
    p, t = flat_pair()
    want = vif_per_image(p.double(), t.double())
    got = hip_metrics(p, t, which=("vif",))["vif"].cpu()
    assert torch.isnan(want).all() and torch.isnan(got).all(), (want, got)


def test_identical_images():
    """PSNR inf through the accumulator, SSIM 1 to 1e-12, VIF 1 to 1e-9.  VIF's own eps = 1e-10 keeps g = s_tt / (s_tt + eps) below one,
    so the float64 definition itself gives 1 - VIF ~ 2 eps / s_tt for an identical pair, a matter of the pixel scale: 7e-12 on a smooth
    synth_image in 0..255 (the scale sigma_n_sq = 2 was defined for; float32 holds it), 6e-9 on the same image in [0, 1] (local variance
    ~0.03) and never under 8e-10 in [0, 1], whose variance ends at 0.25.  The 1e-9 bound is therefore checked on the 0..255 image; on the
    [0, 1] image the kernels must agree with the checker."""
    from ultrazoom_amd.metrics import MetricsAccumulator

    t = synth_image(2, 64, 80, seed=3) * 255.0
    got = hip_metrics(t, t)
    print("identical:", got["ssim"].tolist(), (1.0 - got["vif"]).tolist())
    assert got["sq_err"].cpu().tolist() == [0.0, 0.0]
    for v in got["ssim"].cpu().tolist():
        assert abs(v - 1.0) <= 1e-12, v
    for v in got["vif"].cpu().tolist():
        assert abs(v - 1.0) <= 1e-9, v
    acc = MetricsAccumulator()
    acc.update(t.cuda(), t.cuda())
    assert acc.compute()["psnr"] == float("inf")
    _, smooth = pair(2, 64, 80, 0.3)
    got = hip_metrics(smooth, smooth)
    assert got["sq_err"].cpu().tolist() == [0.0, 0.0]
    for v in got["ssim"].cpu().tolist():
        assert abs(v - 1.0) <= 1e-12, v
    assert_close(got["vif"], vif_per_image(smooth.double(), smooth.double()), 1e-9, "vif of an identical smooth pair")


VIEWS = ["channels_last", "hwc_frame", "bgr", "crop", "every_second_image"]


@pytest.mark.parametrize("dt", ["bf16", "u8"])
@pytest.mark.parametrize("kind", VIEWS)
def test_views_give_the_bits_of_a_dense_copy(kind, dt):
    B, H, W = 2, 45, 52
    p, t = (v.cuda() for v in pair(B, H, W, 0.3, dt))
    dense = raw_of(p, t)
    assert dense[:, 6].abs().min() > 0 and dense[:, 11].abs().min() > 0
    elem = {"bf16": 1, "u8": 3}[dt]

    def as_view(x):
        if kind == "channels_last":
            v = x.contiguous(memory_format=torch.channels_last)
            assert v.stride() == (3 * H * W, 1, 3 * W, 3)
            return v, v.data_ptr(), v.stride()
        if kind == "hwc_frame":
            frame = x.permute(0, 2, 3, 1).contiguous()  # [B, H, W, 3]
            v = frame.permute(0, 3, 1, 2)
            return frame, v.data_ptr(), v.stride()
        if kind == "bgr":
            frame = x.flip(1).permute(0, 2, 3, 1).contiguous()  # [B, H, W, 3] holding B, G, R
            return frame, frame.data_ptr() + 2 * frame.element_size(), (H * W * 3, -1, W * 3, 3)
        if kind == "crop":
            big = torch.full((B, 3, H + 7, W + 9), 0.77, device="cuda").to(x.dtype)
            big[:, :, 3:3 + H, 5:5 + W] = x
            v = big[:, :, 3:3 + H, 5:5 + W]
            return big, v.data_ptr(), v.stride()
        big = torch.full((2 * B, 3, H, W), 0.33, device="cuda").to(x.dtype)
        big[::2] = x
        v = big[::2]
        return big, v.data_ptr(), v.stride()

    keep_p, p_ptr, p_strides = as_view(p)
    keep_t, t_ptr, t_strides = as_view(t)
    got = raw(p_ptr, p_strides, t_ptr, t_strides, elem, B, H, W)
    assert torch.equal(got, dense), (kind, got, dense)
    # a view against a dense image, too
    assert torch.equal(raw(p_ptr, p_strides, t.data_ptr(), t.stride(), elem, B, H, W), dense)


def test_image_stride_beyond_2_to_31_elements():
    """Two 16 x 16 bf16 images inside one flat allocation, 2^31 + 40 elements apart: only the two windows are ever touched."""
    B, H, W = 2, 16, 16
    p, t = (v.cuda() for v in pair(B, H, W, 0.3, "bf16"))
    step = 2**31 + 40
    flat = torch.empty(step + 3 * H * W + 64, dtype=torch.bfloat16, device="cuda")
    far = flat.as_strided((B, 3, H, W), (step, H * W, W, 1), 24)
    far.copy_(p)
    want = raw_of(p, t, which=3)
    got = raw_of(far, t, which=3)
    assert torch.equal(got, want), (got, want)
    got = raw_of(t, far, which=3)
    assert torch.equal(got, raw_of(t, p, which=3))


def test_two_calls_give_the_same_bits_and_images_do_not_depend_on_their_batch():
    B, H, W = 3, 59, 77
    p, t = (v.cuda() for v in pair(B, H, W, 0.3))
    first, second = raw_of(p, t), raw_of(p, t)
    assert torch.equal(first, second)
    fixed = raw_of(p, t, data_range=1.0)
    for i in range(B):
        alone = raw_of(p[i:i + 1], t[i:i + 1], data_range=1.0)
        assert torch.equal(alone[0], fixed[i]), (i, alone[0], fixed[i])
    # data_range=None is the BATCH's range: image 1 (values in [0, 0.5]) alone has another one
    assert float(raw_of(p[1:2], t[1:2])[0, 14]) < 0.75 * float(first[1, 14])


def test_accumulator_matches_the_classes_of_evaluate():
    from ultrazoom_amd.metrics import MetricsAccumulator

    updates = [pair(2, 48, 64, 0.3, "bf16"), pair(1, 41, 57, 0.05, "bf16", seed=21)]
    acc = MetricsAccumulator()
    psnr, ssim, vif = PSNR(1.0), SSIM(), VIF()
    for p, t in updates:
        acc.update(p.cuda(), t.cuda())
        psnr.update(as_double(p), as_double(t))
        ssim.update(as_double(p), as_double(t))
        vif.update(as_double(p), as_double(t))
    got = acc.compute()
    print(got, psnr.compute(), ssim.compute(), vif.compute())
    assert math.isclose(got["psnr"], psnr.compute(), rel_tol=1e-12)
    assert math.isclose(got["ssim"], ssim.compute(), rel_tol=1e-9)
    assert math.isclose(got["vif"], vif.compute(), rel_tol=1e-9)
    small = MetricsAccumulator()
    small.update(*(v.cuda() for v in pair(1, 12, 13, 0.3)))
    assert small.compute()["vif"] is None  # below 41 pixels, as evaluate()


def test_evaluate_hip_backend_matches_the_torch_backend():
    from golden_util import GoldenCase
    from ultrazoom_amd import MewZoom

    case = GoldenCase("g1_2x_c16")
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    m = m.to("cuda").eval()
    x = synth_image(2, 40, 56, seed=6)
    near = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    y = (near + 0.1 * (synth_image(2, 80, 112, seed=7) - 0.5)).clamp(0, 1)  # an independently perturbed image, not the model's output

    class Copies:  # the torch backend fed with CPU copies of the same upscale results
        def upscale(self, x_cpu):
            return m.upscale(x_cpu.cuda()).cpu()

    got = evaluate(m, [(x.cuda(), y.cuda())], backend="hip")
    want = evaluate(Copies(), [(x, y)], backend="torch")
    print(got, want)
    assert got["images"] == want["images"] == 2
    assert math.isclose(got["psnr"], want["psnr"], rel_tol=1e-12)
    assert math.isclose(got["ssim"], want["ssim"], rel_tol=1e-9)
    assert math.isclose(got["vif"], want["vif"], rel_tol=1e-9)


def test_refusals_leave_the_library_usable():
    from ultrazoom_amd.metrics import image_metrics

    p, t = (v.cuda() for v in pair(1, 64, 80, 0.3))
    with pytest.raises(ValueError, match="one shape"):
        image_metrics(p, t[:, :, :-1])
    with pytest.raises(TypeError, match="same dtype"):
        image_metrics(p, t.half())
    with pytest.raises(ValueError, match="11"):
        image_metrics(p[:, :, :10, :30], t[:, :, :10, :30], which=("psnr", "ssim"))
    with pytest.raises(ValueError, match="41"):
        image_metrics(p[:, :, :40], t[:, :, :40])
    with pytest.raises(_ffi.MewZoomHipError):  # the C entry refuses the same on its own
        raw_of(p[:, :, :40], t[:, :, :40], which=4)
    want = reference(1, 64, 80, 0.3, "f32", None, True)
    got = image_metrics(p, t)
    assert_close(got["ssim"], want["ssim"], 1e-9, "ssim")
    assert_close(got["vif"], want["vif"], 1e-9, "vif")


# ---- nothing outside the images is read, nothing outside out and the workspace written (tests/poison_util.py) ------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(2 * TILE_H + 1 + 10, 2 * TILE_W + 1 + 10), (42, 57)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_crop_inside_a_nan_frame_gives_the_bits_of_a_dense_copy(shape, dt):
    """The `crop` view again, the pair inside a larger tensor of NaN instead of 0.77: a halo that reaches over the image's edge, at
    the tile edges of the SSIM map and at the smallest VIF sizes, turns a sum into NaN."""
    B, (H, W) = 2, shape
    p, t = (v.cuda() for v in pair(B, H, W, 0.3, dt))
    dense = raw_of(p, t)
    assert not bool(torch.isnan(dense).any()) and dense[:, 6].abs().min() > 0 and dense[:, 11].abs().min() > 0

    def framed(x):
        big = torch.full((B, 3, H + 7, W + 9), float("nan"), device="cuda").to(x.dtype)
        big[:, :, 3:3 + H, 5:5 + W] = x
        return big, big[:, :, 3:3 + H, 5:5 + W]

    (keep_p, pv), (keep_t, tv) = framed(p), framed(t)
    assert torch.equal(raw_of(pv, tv), dense)
    assert torch.equal(raw_of(pv, t), dense) and torch.equal(raw_of(p, tv), dense)


@pytest.mark.parametrize("which", [7, 3, 4])
def test_a_poisoned_workspace_and_the_slots_that_are_not_asked_for(which):
    """The workspace starts as 0xFF bytes (NaN as float64) between pattern guards, the images sit between NaN guards: the same bits as
    on a fresh workspace, no guard touched, and the `out` slots of the metrics that `which` leaves out keep what they held."""
    from poison_util import Arena

    B, H, W = 2, 45, 52
    p, t = (v.cuda() for v in pair(B, H, W, 0.3, "bf16"))
    dense = raw_of(p, t, which=which)
    written = sorted(([0, 1, 2, 3, 4, 5] if which & 1 else []) + ([0, 1, 2, 3, 4, 5, 6, 7, 14] if which & 2 else [])
                     + ([8, 9, 10, 11, 12, 13] if which & 4 else []))  # (SSIM of data_range=None takes the batch's range from the PSNR pass)
    written = sorted(set(written))
    kept = [s for s in range(_ffi.MZ_METRIC_SLOTS) if s not in written]
    need = _ffi.metrics_workspace_bytes(B, H, W, which)
    arena = Arena("cuda")
    pa, ta = arena.input(p, name="pred"), arena.input(t, name="target")
    out = arena.output((B, _ffi.MZ_METRIC_SLOTS), torch.float64, fill=-1.0, name="out")
    ws = arena.raw(need, 0xFF, name="workspace")
    _ffi.metrics(pa.data_ptr(), pa.stride(), ta.data_ptr(), ta.stride(), 1, B, H, W, which, -1.0, 2.0, out.data_ptr(), ws.data_ptr(), need,
                 torch.cuda.current_stream().cuda_stream)
    arena.check()
    assert not bool(torch.isnan(out).any()), out
    assert torch.equal(out[:, written], dense[:, written]), (out, dense)
    assert bool((out[:, kept] == -1.0).all()), f"slots {kept} are not {which}'s to write: {out}"
