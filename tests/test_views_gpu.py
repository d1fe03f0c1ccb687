"""Images as views at both ends (mz_forward_view, MewZoom.upscale_into, zero-copy upscale_tiled).

A view changes addresses, never arithmetic: every comparison with the dense path -- today's `upscale` / `upscale_uint8` on a contiguous
copy of the same pixels -- is `torch.equal`.  Models are the tiny fixtures of tests/golden; "u8" runs uint8 images through the bf16
model (the 256-pixel image head), "u8f32" through the f32 model (the 512-pixel one)."""

import functools

import pytest
import torch

from golden_util import GoldenCase
from op_util import selected, set_knobs
from ultrazoom_amd import MewZoom, _ffi
from ultrazoom_amd.synth import synth_image, synth_state_dict
from ultrazoom_amd.tiling import receptive_field, upscale_tiled

pytestmark = pytest.mark.gpu

MODEL_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.bfloat16, "u8f32": torch.float32}
KINDS = sorted(MODEL_DTYPE)
SENTINEL = 77  # no result of a clamped float path; for uint8 just "not written": the dense values next to it are compared anyway


@functools.lru_cache(maxsize=None)
def model(name: str, kind: str) -> MewZoom:
    case = GoldenCase(name)
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    return m.to("cuda", MODEL_DTYPE[kind]).eval()


def image(kind: str, B: int, H: int, W: int, seed: int) -> torch.Tensor:
    x = synth_image(B, H, W, seed=seed)
    if kind.startswith("u8"):
        return (x * 255.0).round().to(torch.uint8).cuda()
    return x.to("cuda", MODEL_DTYPE[kind])


@functools.lru_cache(maxsize=None)
def pixels_and_dense(name: str, kind: str, B: int, H: int, W: int, seed: int):
    """A contiguous image and the dense result for it, computed once and shared (never written to)."""
    m = model(name, kind)
    x = image(kind, B, H, W, seed)
    return x, (m.upscale_uint8(x) if kind.startswith("u8") else m.upscale(x))


def sentinel_like(x: torch.Tensor, shape) -> torch.Tensor:
    return torch.full(shape, SENTINEL, dtype=x.dtype, device=x.device)


def crop_of(x: torch.Tensor, top: int, left: int, bottom: int = 6, right: int = 6):
    """(the larger sentinel buffer, its crop holding x's pixels, the mask of the crop)"""
    B, C, H, W = x.shape
    big = sentinel_like(x, (B, C, H + top + bottom, W + left + right))
    big[:, :, top : top + H, left : left + W] = x
    mask = torch.zeros(big.shape, dtype=torch.bool, device=x.device)
    mask[:, :, top : top + H, left : left + W] = True
    return big, big[:, :, top : top + H, left : left + W], mask


def input_view(x: torch.Tensor, layout: str) -> torch.Tensor:
    if layout == "channels_last":
        v = x.contiguous(memory_format=torch.channels_last)
    elif layout == "crop":  # row pitch != W, the base aligned to one element only (3 rows + 5 columns of an odd pitch)
        v = crop_of(x, 3, 5)[1]
    else:  # images 1 and 3 of a five-image batch
        big = sentinel_like(x, (5,) + tuple(x.shape[1:]))
        big[1::2] = x
        v = big[1::2]
    assert not v.is_contiguous() and torch.equal(v, x)
    return v


# ---- 1. input views -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channels_last", "crop", "batch"])
@pytest.mark.parametrize("kind", KINDS)
def test_input_views_equal_dense(kind, layout):
    m = model("g1_2x_c16", kind)
    x, dense = pixels_and_dense("g1_2x_c16", kind, 2, 37, 45, 41)
    v = input_view(x, layout)
    out = sentinel_like(dense, dense.shape)
    assert m.upscale_into(v, out) is out
    assert torch.equal(out, dense)
    # the public methods take the view as it is, and still return dense NCHW
    got = m.upscale_uint8(v) if kind.startswith("u8") else m.upscale(v)
    assert got.is_contiguous() and torch.equal(got, dense)


@pytest.mark.parametrize("name", ["g3_4x_c16", "g4_8x_c16"])
@pytest.mark.parametrize("kind", KINDS)
def test_cropped_input_equals_dense_at_4x_and_8x(kind, name):
    case = GoldenCase(name)
    m = model(name, kind)
    x, dense = pixels_and_dense(name, kind, case.B, case.H, case.W, 42)
    got = m.upscale_uint8(input_view(x, "crop")) if kind.startswith("u8") else m.upscale(input_view(x, "crop"))
    assert torch.equal(got, dense)


def test_forward_and_predict_degredation_take_views():
    m = model("g1_2x_c16", "bf16")
    x, _ = pixels_and_dense("g1_2x_c16", "bf16", 2, 37, 45, 41)
    v = input_view(x, "channels_last")
    sr, qa = m.forward(x)
    sr_v, qa_v = m.forward(v)
    assert torch.equal(sr_v, sr) and torch.equal(qa_v, qa) and torch.equal(m.predict_degredation(v), qa)


# ---- 2. output views ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_output_views_equal_dense_and_leave_the_rest_alone(kind):
    m = model("g1_2x_c16", kind)
    x, dense = pixels_and_dense("g1_2x_c16", kind, 2, 37, 45, 41)
    out = sentinel_like(dense, dense.shape).contiguous(memory_format=torch.channels_last)
    m.upscale_into(x, out)
    assert not out.is_contiguous() and torch.equal(out, dense)
    big, out, mask = crop_of(sentinel_like(dense, dense.shape), 2, 3, bottom=5, right=7)
    m.upscale_into(x, out)
    assert torch.equal(out, dense)
    assert bool((big[~mask] == SENTINEL).all()), "an element outside the output view was written"


# ---- 3. windows ---------------------------------------------------------------------------------------------------------------
def check_window(m, x, dense, window):
    y0, x0, h, w = window
    big, out, mask = crop_of(sentinel_like(dense, (dense.shape[0], 3, h, w)), 2, 3, bottom=5, right=7)
    m.upscale_into(x, out, window=window)
    assert torch.equal(out, dense[:, :, y0 : y0 + h, x0 : x0 + w]), window
    assert bool((big[~mask] == SENTINEL).all()), f"window {window}: an element outside the output view was written"


@pytest.mark.parametrize("window", [(3, 5, 2 * 37 - 7, 2 * 45 - 6), (2 * 37 - 1, 2 * 45 - 1, 1, 1), (0, 0, 21, 70)],
                         ids=["inner", "last_pixel", "origin_to_mid_tile"])
@pytest.mark.parametrize("kind", KINDS)
def test_window_of_2x_equals_that_part_of_dense(kind, window):
    x, dense = pixels_and_dense("g1_2x_c16", kind, 2, 37, 45, 41)
    check_window(model("g1_2x_c16", kind), x, dense, window)


@pytest.mark.parametrize("kind", KINDS)
def test_one_pixel_window_at_the_last_output_pixel_of_an_8x9_image(kind):
    """The smallest image the model takes but for one column (levels 8 x 9, 4 x 4, 2 x 2, 1 x 1), the smallest window, the largest origin."""
    x, dense = pixels_and_dense("g1_2x_c16", kind, 2, 8, 9, 43)
    assert dense.shape == (2, 3, 16, 18)
    check_window(model("g1_2x_c16", kind), x, dense, (15, 17, 1, 1))
    out = sentinel_like(dense, dense.shape)
    model("g1_2x_c16", kind).upscale_into(x, out)
    assert torch.equal(out, dense)


@pytest.mark.parametrize("kind", KINDS)
def test_window_of_4x_with_an_odd_origin(kind):
    case = GoldenCase("g3_4x_c16")
    x, dense = pixels_and_dense("g3_4x_c16", kind, case.B, case.H, case.W, 42)
    rH, rW = dense.shape[-2:]
    check_window(model("g3_4x_c16", kind), x, dense, (5, 7, rH - 5 - 9, rW - 7 - 3))  # 5, 7: odd, no multiple of 4
    check_window(model("g3_4x_c16", kind), x, dense, (rH - 1, rW - 1, 1, 1))


# ---- 4. micro-batches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "u8"])
def test_micro_batches_advance_the_views_by_their_image_stride(kind):
    m = model("g1_2x_c16", kind)
    x, dense = pixels_and_dense("g1_2x_c16", kind, 5, 37, 45, 43)
    xin = crop_of(x, 0, 0, bottom=1, right=0)[1]           # image stride 3 * 38 * 45 > one image
    big, out, mask = crop_of(sentinel_like(dense, dense.shape), 0, 0, bottom=3, right=0)
    assert xin.stride(0) > 3 * 37 * 45 and out.stride(0) > dense.stride(0)
    m.max_images_in_flight = 2
    try:
        m.upscale_into(xin, out)
    finally:
        m.max_images_in_flight = 0
    assert torch.equal(out, dense)
    assert bool((big[~mask] == SENTINEL).all())


# ---- 5. signed strides, through _ffi ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16", "u8"])
def test_negative_channel_strides_are_bgr(kind):
    m = model("g1_2x_c16", kind)
    x, _ = pixels_and_dense("g1_2x_c16", kind, 2, 37, 45, 41)
    flipped = x.flip(1).contiguous()
    want = (m.upscale_uint8(flipped) if kind.startswith("u8") else m.upscale(flipped)).flip(1)
    B, _, H, W = x.shape
    out = sentinel_like(want, want.shape)
    engine = m._get_engine(torch.empty(0, dtype=MODEL_DTYPE[kind], device=x.device))
    stream = torch.cuda.current_stream()
    ws = engine._workspace_for(engine.handle.workspace_bytes(B, H, W, 0), stream)
    engine.handle.forward_view(
        x.data_ptr() + 2 * x.stride(1) * x.element_size(), (x.stride(0), -x.stride(1), W, 1),
        out.data_ptr() + 2 * out.stride(1) * out.element_size(), (out.stride(0), -out.stride(1), out.stride(2), 1),
        0, B, H, W, True, 1 if kind.startswith("u8") else 0, None, ws.data_ptr(), ws.numel(), 0, stream.cuda_stream,
    )
    engine._mark_done(stream)
    assert torch.equal(out, want)


# ---- 6. 64-bit offsets --------------------------------------------------------------------------------------------------------
def test_output_rows_beyond_4_gib():
    """66 output rows at a pitch of 2^26 + 64 bytes: rows 64 and 65 start beyond 2^32 bytes from the view's first element."""
    m = model("g1_2x_c16", "u8")
    x, dense = pixels_and_dense("g1_2x_c16", "u8", 1, 33, 45, 44)
    pitch = 2**26 + 64
    buf = torch.empty(4_400_000_000, dtype=torch.uint8, device="cuda")
    out = torch.as_strided(buf, (1, 3, 66, 90), (270, 90, pitch, 1))
    assert 65 * pitch > 2**32 and 65 * pitch + 270 <= buf.numel()
    m.upscale_into(x, out)
    assert torch.equal(out, dense)


# ---- 7. against the reference -------------------------------------------------------------------------------------------------
def test_views_against_the_reference_fixture():
    case = GoldenCase("g1_2x_c16")
    m = model("g1_2x_c16", "f32")
    x = case.image().to("cuda", torch.float32).contiguous(memory_format=torch.channels_last)
    r = case.config["upscale_ratio"]
    _, out, _ = crop_of(torch.zeros(case.B, 3, r * case.H, r * case.W, device="cuda"), 2, 3)
    m.upscale_into(x, out)
    err = case.compare_sr(out, out)["up"]
    assert err <= 1e-3, f"upscale_into through views deviates from the reference fixture by {err:.3e}"


# ---- 8. tiling ----------------------------------------------------------------------------------------------------------------
def test_tiled_uint8_equals_upscale_uint8():
    m = model("g1_2x_c16", "u8")
    x = image("u8", 2, 203, 277, 13)
    assert torch.equal(upscale_tiled(m, x, tile=(64, 120)), m.upscale_uint8(x))


@pytest.fixture
def calls(monkeypatch):
    """Counts the library entries a test goes through."""
    n = {"view": 0, "dense": 0}
    view, dense = _ffi.Handle.forward_view, _ffi.Handle.forward

    def counted_view(self, *a, **k):
        n["view"] += 1
        return view(self, *a, **k)

    def counted_dense(self, *a, **k):
        n["dense"] += 1
        return dense(self, *a, **k)

    monkeypatch.setattr(_ffi.Handle, "forward_view", counted_view)
    monkeypatch.setattr(_ffi.Handle, "forward", counted_dense)
    return n


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_tiling_makes_one_view_call_per_tile_and_no_dense_call(kind, calls):
    m = model("g1_2x_c16", kind)
    x = image(kind, 2, 203, 277, 13)  # odd sizes: floors and pads at every level
    full = m.upscale(x)
    assert calls == {"view": 0, "dense": 1}
    tiled = upscale_tiled(m, x, tile=(64, 120))
    assert calls == {"view": 4 * 3, "dense": 1}  # ceil(203 / 64) x ceil(277 / 120) tiles
    assert torch.equal(tiled, full)


def test_a_model_with_upscale_only_still_gets_dense_calls(calls):
    m = model("g1_2x_c16", "bf16")

    class OnlyUpscale:
        _cfg = m._cfg

        def upscale(self, t):
            assert t.is_contiguous()
            return m.upscale(t)

    x = image("bf16", 1, 203, 277, 13)
    tiled = upscale_tiled(OnlyUpscale(), x, tile=(64, 120))
    assert calls == {"view": 0, "dense": 4 * 3}
    assert torch.equal(tiled, m.upscale(x))


# ---- 9. 16-bit tiles of a 48-channel, hidden-ratio-2 model run the kernels the whole image runs -------------------------------
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_tiled_equals_untiled_48_channels_hidden_ratio_2(kind):
    """The level-1 blocks of the 48-channel models: conv1 on conv3r_kernel's ragged variant, conv2 + mix on conv3t_kernel's fused one.
    Both sum in another order than the kernels they replace, so a tile must choose them exactly as the whole image does: the choice
    is asserted for the image and for the centre tile's slice (mz_debug_select runs the function the launches run), the result
    bit for bit."""
    cfg = dict(upscale_ratio=2, primary_channels=48, primary_layers=2, secondary_channels=96, secondary_layers=2,
               tertiary_channels=96, tertiary_layers=2, quaternary_channels=96, quaternary_layers=2, hidden_ratio=2, num_deg_features=3)
    m = MewZoom(**cfg)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=5))
    m = m.to("cuda", MODEL_DTYPE[kind]).eval()
    halo = receptive_field(cfg)
    H, W, tile = 2 * 104 + halo + 16, 2 * 104 + halo + 24, (104, 104)
    assert all(t > halo and n > 2 * t + halo for t, n in zip(tile, (H, W))), "the centre tile must be cut on all four sides"
    cus = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    for h, w in ((H, W), (tile[0] + 2 * halo, tile[1] + 2 * halo)):
        assert selected("conv", (1, h, w, 48, 96, 1), kind, cus=cus) == "conv3r_ragged"
        assert selected("conv_mix", (1, h, w, 96, 48), kind, cus=cus) == "conv3t_fused"
    x = image(kind, 1, H, W, 32)
    assert torch.equal(upscale_tiled(m, x, tile=tile), m.upscale(x))


def test_f32_views_on_the_256_pixel_kernel(monkeypatch):
    """MZ_NO_WIDE=1 keeps the f32 image head on conv_kernel: its view instantiation against its dense one."""
    set_knobs(monkeypatch, {"MZ_NO_WIDE": "1"})
    case = GoldenCase("g1_2x_c16")
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    m = m.to("cuda", torch.float32).eval()  # a model of its own: the knobs are read when its handle is created
    x = image("f32", 2, 37, 45, 41)
    dense = m.upscale(x)
    big, out, mask = crop_of(sentinel_like(dense, (2, 3, 2 * 37 - 7, 2 * 45 - 6)), 2, 3)
    m.upscale_into(input_view(x, "crop"), out, window=(3, 5, 2 * 37 - 7, 2 * 45 - 6))
    assert torch.equal(out, dense[:, :, 3 : 2 * 37 - 4, 5 : 2 * 45 - 1])
    assert bool((big[~mask] == SENTINEL).all())


# ---- upscale_into refuses what it cannot run ----------------------------------------------------------------------------------
def test_upscale_into_refuses_wrong_device_dtype_and_shape():
    m = model("g1_2x_c16", "bf16")
    x, dense = pixels_and_dense("g1_2x_c16", "bf16", 2, 37, 45, 41)
    good = torch.empty_like(dense)
    for bad_x, bad_out, window in (
        (x.cpu(), good, None),                                    # no CPU path
        (x, good.cpu(), None),                                    # the output elsewhere
        (x.float(), good.float(), None),                          # not the module's dtype
        (x, good.float(), None),                                  # two dtypes
        (x, good.to(torch.uint8), None),                          # uint8 on one side only
        (x, good[:, :, :-1], None),                               # not [B, 3, rH, rW]
        (x, good, (0, 0, 10, 10)),                                # not the window's shape
        (x[:, :2], good, None),                                   # not three channels
    ):
        with pytest.raises(RuntimeError):
            m.upscale_into(bad_x, bad_out, window=window)
    with pytest.raises(_ffi.MewZoomHipError):                     # the library's own check: a window outside the output
        m.upscale_into(x, good[:, :, :10, :10], window=(70, 0, 10, 10))
