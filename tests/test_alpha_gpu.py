"""mz_alpha_fill, mz_alpha_merge and upscale_rgba on the GPU against the restatement of ultrazoom_amd/csrc/mz_alpha.h (tests/alpha_ref.py),
bit for bit: every size at which the pyramid takes another shape (one pixel, one row, one column, odd sides, several workgroups), the
four element types, straight and premultiplied input, every layout the views describe; the colour under a == 0 changes no bit; a
one-colour image comes back exactly; the merged alpha has the bits of `interpolate` on the plane; the model between the two."""

import functools

import pytest
import torch

import alpha_ref
from alpha_ref import DTYPES, SIZES, same_bits
from model_util import lower_built
from ultrazoom_amd import _ffi, alpha_fill, alpha_merge, interpolate, upscale_rgba
from ultrazoom_amd.tiling import upscale_tiled

pytestmark = pytest.mark.gpu

B = 2


@functools.lru_cache(maxsize=None)
def case(H, W, dt, premultiplied, kind="mixed"):
    """(the RGBA batch on the CPU, the expected fill): computed once, left unchanged"""
    x = alpha_ref.rgba(B, H, W, dt, kind=kind)
    if premultiplied:
        x = alpha_ref.premultiplied_of(x, dt)
    return x, alpha_ref.fill_expected(x[:, :3], x[:, 3:4], dt, premultiplied)


def layouts(x):
    """name -> (rgb, alpha) views on the GPU of the CPU batch x [B, 4, H, W]"""
    Bx, _, H, W = x.shape
    planar = x.cuda()
    hwc = x.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)  # an interleaved RGBA buffer: two views, three elements apart
    frame = (torch.rand((Bx, 4, H + 5, W + 9)) * 255).to(x.dtype).cuda()   # a crop of a larger frame of other values
    frame[:, :, 2:2 + H, 3:3 + W] = planar
    crop = frame[:, :, 2:2 + H, 3:3 + W]
    return {"planar": (planar[:, :3], planar[:, 3:4]), "hwc": (hwc[:, :3], hwc[:, 3:4]),
            "separate": (x[:, :3].contiguous().cuda(), x[:, 3:4].contiguous().cuda()), "crop": (crop[:, :3], crop[:, 3:4])}


# ---- the fill -----------------------------------------------------------------------------------------------------------------------------
def _fill_equals_the_restatement_bit_for_bit(H, W, dt):
    for premultiplied in (False, True):
        x, want = case(H, W, dt, premultiplied)
        for name, (rgb, alpha) in layouts(x).items():
            got = alpha_fill(rgb, alpha, premultiplied=premultiplied)
            assert got.is_contiguous() and same_bits(got, want), (name, premultiplied)
        # into a view: the rgb part of an interleaved result (the element-store path), from planar input
        rgb, alpha = layouts(x)["planar"]
        buf = torch.zeros((B, H, W, 4), dtype=DTYPES[dt], device="cuda")
        out = buf.permute(0, 3, 1, 2)[:, :3]
        assert alpha_fill(rgb, alpha, premultiplied=premultiplied, out=out) is out
        assert same_bits(out.contiguous(), want) and bool((buf[..., 3] == 0).all()), premultiplied


@pytest.mark.parametrize("H, W", SIZES, ids=lambda v: str(v))
def test_fill_equals_the_restatement_bit_for_bit(H, W):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _fill_equals_the_restatement_bit_for_bit(H, W, dt)


def _the_colour_under_zero_alpha_changes_no_bit(H, W, dt):
    for premultiplied in (False, True):
        x, want = case(H, W, dt, premultiplied)
        for what in ("nan", "inf", "random"):
            g = alpha_ref.garbage(x, dt, what).cuda()
            assert same_bits(alpha_fill(g[:, :3], g[:, 3:4], premultiplied=premultiplied), want), (what, premultiplied)
        if not premultiplied:  # visible pixels come back as the bit patterns that went in
            seen = torch.from_numpy(alpha_ref.alpha_values(x[:, 3:4]) > 0).expand(-1, 3, -1, -1)
            got = alpha_fill(x[:, :3].cuda(), x[:, 3:4].cuda()).cpu()
            assert same_bits(got[seen], x[:, :3][seen])


@pytest.mark.parametrize("H, W", [(5, 3), (17, 33), (64, 48)], ids=lambda v: str(v))
def test_the_colour_under_zero_alpha_changes_no_bit(H, W):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _the_colour_under_zero_alpha_changes_no_bit(H, W, dt)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_an_opaque_image_comes_back_whole_and_a_clear_one_as_zeros(dt):
    for H, W in ((1, 1), (9, 8), (17, 33)):
        x = alpha_ref.rgba(B, H, W, dt, kind="opaque").cuda()
        assert same_bits(alpha_fill(x[:, :3], x[:, 3:4]), x[:, :3].contiguous())
        clear = alpha_ref.garbage(alpha_ref.rgba(B, H, W, dt, kind="clear"), dt, "nan").cuda()
        got = alpha_fill(clear[:, :3], clear[:, 3:4])
        assert same_bits(got, torch.zeros_like(got))


def _a_constant_comes_back_exactly(H, W, dt):
    """binary alpha, one float32-representable colour per channel on the visible pixels: every output pixel is that colour exactly"""
    x = alpha_ref.rgba(B, H, W, dt, kind="binary").clone()
    colour = torch.tensor([0.3, 0.6015625, 1.0], dtype=torch.float64)
    colour = (colour * 255 + 0.5).to(torch.uint8) if dt == "u8" else colour.to(DTYPES[dt])
    x[:, :3] = colour.view(1, 3, 1, 1)
    noisy = alpha_ref.garbage(x, dt, "random").cuda()
    assert same_bits(alpha_fill(noisy[:, :3], noisy[:, 3:4]), x[:, :3].contiguous())


@pytest.mark.parametrize("H, W", [(9, 8), (17, 33)], ids=lambda v: str(v))
def test_a_constant_comes_back_exactly(H, W):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _a_constant_comes_back_exactly(H, W, dt)


# ---- the merge ----------------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [((8, 8), (16, 16)), ((8, 8), (32, 32)), ((8, 8), (64, 64)), ((9, 11), (18, 22)), ((9, 11), (36, 44)), ((9, 11), (72, 88)),
                ((9, 11), (20, 31))]


def _merge_equals_interpolate_on_the_plane_and_the_product_rounded_once(shape, dt):
    (H, W), size = shape
    x = alpha_ref.rgba(B, H, W, dt)
    alpha = x[:, 3:4].cuda()
    sr_cpu = alpha_ref.rgba(B, size[0], size[1], dt, seed=23)[:, :3].contiguous()
    sr = sr_cpu.cuda()
    for mode in alpha_ref.MODES:
        plane = interpolate(alpha.expand(B, 3, H, W), size=size, mode=mode, clamp=mode != "nearest")[:, :1]  # (nearest takes no clamp)
        want_alpha, want_rgb = alpha_ref.merge_expected(sr_cpu, x[:, 3:4], size, mode, dt, True)
        plain = alpha_merge(sr, alpha, size=size, mode=mode)
        assert same_bits(plain[:, 3:4].contiguous(), plane.contiguous()) and same_bits(plane.contiguous(), want_alpha), mode
        assert same_bits(plain[:, :3].contiguous(), sr_cpu), mode           # without premultiply the colour is stored as it is
        pre = alpha_merge(sr, alpha, size=size, mode=mode, premultiply=True)
        assert same_bits(pre[:, 3:4].contiguous(), want_alpha) and same_bits(pre[:, :3].contiguous(), want_rgb), mode
        assert torch.equal(sr.cpu(), sr_cpu)                                 # (a separate result: the colour that went in is not written)
        # in place in an interleaved buffer: the same bits
        buf = torch.zeros((B, size[0], size[1], 4), dtype=DTYPES[dt], device="cuda")
        out = buf.permute(0, 3, 1, 2)
        out[:, :3] = sr
        assert alpha_merge(out[:, :3], alpha, size=size, mode=mode, premultiply=True, out=out) is out
        assert same_bits(out.contiguous(), pre), mode


@pytest.mark.parametrize("shape", MERGE_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}to{v[1][0]}x{v[1][1]}")
def test_merge_equals_interpolate_on_the_plane_and_the_product_rounded_once(shape):
    for dt in sorted(DTYPES):  # (one test for the four element types: a failure's traceback names dt)
        _merge_equals_interpolate_on_the_plane_and_the_product_rounded_once(shape, dt)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_without_premultiply_a_poisoned_out_rgb_is_untouched(dt):
    H, W, size = 9, 11, (20, 31)
    alpha = alpha_ref.rgba(B, H, W, dt)[:, 3:4].cuda()
    raw = torch.full((B, 4, size[0], size[1] * DTYPES[dt].itemsize), 0xFF, dtype=torch.uint8, device="cuda")
    out = raw.view(DTYPES[dt])  # [B, 4, Hout, Wout] of all-ones bytes
    before = out.clone()
    stream = torch.cuda.current_stream().cuda_stream
    for views in ((_ffi.pair(out[:, :3]), _ffi.pair(out[:, :3])), (None, None)):
        _ffi.alpha_merge(views[0], _ffi.pair(alpha), views[1], _ffi.pair(out[:, 3:4]), alpha_ref.ELEM[dt], B, H, W, size[0], size[1], 2, False, stream)
        assert torch.equal(out[:, :3].contiguous().view(torch.uint8), before[:, :3].contiguous().view(torch.uint8))
    want, _ = alpha_ref.merge_expected(None, alpha.cpu(), size, "bicubic", dt, False)
    assert same_bits(out[:, 3:4].contiguous(), want)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def model_input(H, W, dt, kind):
    return alpha_ref.rgba(B, H, W, dt, seed=31, kind=kind).cuda()


def plain_upscale(model, rgb):
    rgb = rgb.contiguous()
    return model.upscale_uint8(rgb) if rgb.dtype == torch.uint8 else model.upscale(rgb)


@pytest.mark.parametrize("dt", ["bf16", "u8"])
@pytest.mark.parametrize("name, r", [("g1", 2), ("g3", 4), ("g4", 8)])
def test_an_opaque_image_is_upscale_of_its_colour_with_an_alpha_of_exactly_one(name, r, dt):
    model = lower_built(name, torch.bfloat16)
    x = model_input(8, 12, dt, "opaque")
    for mode in alpha_ref.MODES:
        got = model.upscale_rgba(x, alpha_mode=mode)
        assert tuple(got.shape) == (B, 4, 8 * r, 12 * r) and got.dtype == x.dtype
        assert same_bits(got[:, :3].contiguous(), plain_upscale(model, x[:, :3]))
        assert bool((got[:, 3] == (255 if dt == "u8" else 1)).all()), mode


@pytest.mark.parametrize("dt, model_dtype", [("bf16", torch.bfloat16), ("f32", torch.float32), ("u8", torch.bfloat16)])
@pytest.mark.parametrize("premultiplied", [False, True])
def test_upscale_rgba_is_the_three_public_calls(dt, model_dtype, premultiplied):
    model = lower_built("g1", model_dtype)  # 2X
    H, W, r = 11, 16, 2
    x = model_input(H, W, dt, "mixed")
    if premultiplied:
        x = alpha_ref.premultiplied_of(x.cpu(), dt).cuda()
    got = upscale_rgba(model, x, premultiplied=premultiplied, alpha_mode="bilinear")
    sr = plain_upscale(model, alpha_fill(x[:, :3], x[:, 3:4], premultiplied=premultiplied))
    want = alpha_merge(sr, x[:, 3:4], size=(r * H, r * W), mode="bilinear", premultiply=premultiplied)
    assert same_bits(got, want)
    assert same_bits(model.upscale_rgba(x, premultiplied=premultiplied, alpha_mode="bilinear"), want)
    # the colour under a == 0 of the input reaches no bit of the result
    junk = alpha_ref.garbage(x.cpu(), dt, "random").cuda()
    assert same_bits(upscale_rgba(model, junk, premultiplied=premultiplied, alpha_mode="bilinear"), want)


def test_a_permuted_hwc_uint8_buffer_at_both_ends_and_tiles_give_the_plain_result():
    model = lower_built("g1", torch.bfloat16)
    H, W, r = 16, 16, 2
    x = model_input(H, W, "u8", "mixed")
    want = model.upscale_rgba(x)
    decoded = x.permute(0, 2, 3, 1).contiguous()             # [B, H, W, 4], as an image decoder hands it over
    buf = torch.zeros((B, r * H, r * W, 4), dtype=torch.uint8, device="cuda")
    out = buf.permute(0, 3, 1, 2)
    assert model.upscale_rgba(decoded.permute(0, 3, 1, 2), out=out) is out
    assert torch.equal(buf, want.permute(0, 2, 3, 1))
    assert torch.equal(model.upscale_rgba(x, tile=(8, 8)), want)
    xb = model_input(H, W, "bf16", "mixed")
    assert same_bits(model.upscale_rgba(xb, tile=(8, 8)), model.upscale_rgba(xb))
    # (the tiled form is upscale_tiled on the filled colour)
    filled = alpha_fill(xb[:, :3], xb[:, 3:4])
    assert same_bits(model.upscale_rgba(xb)[:, :3].contiguous(), upscale_tiled(model, filled, tile=(8, 8)))


@pytest.mark.parametrize("dt", ["bf16", "u8"])
def test_a_one_colour_disc_on_a_garbage_background_is_upscale_of_the_constant_image(dt):
    """the case the feature exists for: no fringe -- not a small one, none: the bits of the constant image's upscale"""
    model = lower_built("g1", torch.bfloat16)
    H, W = 16, 16
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disc = (((yy - 7.5) ** 2 + (xx - 7.5) ** 2) <= 25.0).view(1, 1, H, W).expand(B, 1, H, W)
    colour = torch.tensor([0.8, 0.25, 0.1], dtype=torch.float64)
    colour = (colour * 255 + 0.5).to(torch.uint8) if dt == "u8" else colour.to(DTYPES[dt])
    const = colour.view(1, 3, 1, 1).expand(B, 3, H, W).contiguous()
    one = torch.tensor(255 if dt == "u8" else 1.0).to(DTYPES[dt])
    x = torch.cat([const, torch.where(disc, one, torch.zeros_like(one))], dim=1)
    want = plain_upscale(model, const.cuda())
    for what in ("nan", "inf", "random"):
        got = model.upscale_rgba(alpha_ref.garbage(x, dt, what).cuda())
        assert same_bits(got[:, :3].contiguous(), want), what
    # and what the feature replaces: dropping alpha lets the garbage through
    dropped = plain_upscale(model, alpha_ref.garbage(x, dt, "random")[:, :3].cuda())
    assert not same_bits(dropped, want)
