"""Feathered tiling on the GPU: mz_feather_paste against the numpy restatement of mz_feather.h (tests/feather_ref.py), bit for bit, on
the 16-byte path and on the element path; its refusals; and ultrazoom_amd.tiling.upscale_feathered -- in the exact regime (a halo that
covers the receptive field plus the overlap: the bits of `upscale`), in the small-halo regime against the reference's strip order on
the tiles the model really gives, and against a derived error bound."""

import functools

import pytest
import torch

import feather_ref
from feather_ref import DTYPES, ELEM, same_bits
from model_util import lower_built
from ultrazoom_amd import _ffi, feather_paste, upscale_feathered
from ultrazoom_amd.synth import synth_image
from ultrazoom_amd.tiling import plan_feathered, receptive_field

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(1, 1), (5, 7), (33, 130), (64, 257)]  # one element; less than a run; ragged runs, two workgroups of rows; three tiles of float32 columns
RAMPS = [(0, 0), (6, 0), (0, 10), (6, 10), (200, 0), (0, 1)]  # none; one axis; both; longer than the rectangle; one position
FILL = {"f32": 7.0, "bf16": 7.0, "f16": 7.0, "u8": 0x5A}


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def carve(buf: torch.Tensor, layout: str, H: int, W: int) -> torch.Tensor:
    """the [B, 3, H, W] view of a buffer of `place`"""
    if layout == "aligned":
        return buf[:, :, :, :W]
    if layout == "crop":
        return buf[:, :, 1 : 1 + H, 3 : 3 + W]
    return buf.permute(0, 3, 1, 2)[:, :3]


def place(t: torch.Tensor, layout: str, dt: str):
    """(a device view that holds t, the whole buffer it lies in, the mask of the buffer's elements outside the view).  "aligned": a row
    pitch of whole 16-byte runs -- rows_aligned holds, the 16-byte path runs; "crop": an odd offset in a larger frame -- the element
    path; "hwc": interleaved, a fourth element a pixel."""
    _, _, H, W = t.shape
    shape = {"aligned": (B, 3, H, (W + 15) // 16 * 16), "crop": (B, 3, H + 3, W + 5), "hwc": (B, H, W, 4)}[layout]
    buf = torch.full(shape, FILL[dt], dtype=t.dtype, device="cuda")
    v = carve(buf, layout, H, W)
    v.copy_(t)
    outside = torch.ones(shape, dtype=torch.bool, device="cuda")
    carve(outside, layout, H, W)[:] = False
    return v, buf, outside


@pytest.mark.parametrize("layout", ["aligned", "crop", "hwc"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_paste_has_the_bits_of_the_reference(dt, layout):
    for H, W in SHAPES:
        for ramp in RAMPS:
            src, dst = feather_ref.pair(B, H, W, dt, ramp)
            want = feather_ref.expected(B, H, W, dt, ramp)
            s, sbuf, _ = place(src, layout, dt)
            d, dbuf, outside = place(dst, layout, dt)
            vec = layout == "aligned"
            assert (s.stride(3) == 1 and s.stride(2) % 16 == 0 and s.data_ptr() % 16 == 0) == vec
            kept = sbuf.clone()
            assert feather_paste(s, d, ramp=ramp) is d
            torch.cuda.synchronize()
            assert same_bits(d.contiguous(), want), (H, W, ramp)
            assert torch.equal(feather_ref.bits(sbuf), feather_ref.bits(kept)), "the paste changed src"
            assert bool((dbuf[outside] == FILL[dt]).all()), "the paste wrote outside dst"


def test_refusals_leave_dst_unchanged():
    H, W = 9, 40
    for dt in ("bf16", "u8"):
        src, dst = (t.cuda() for t in feather_ref.pair(B, H, W, dt, (2, 3)))
        before = dst.clone()
        wide = torch.zeros((B, 3, H, W + 8), dtype=DTYPES[dt], device="cuda")
        wide_before = wide.clone()
        e, p = ELEM[dt], _ffi.pair
        calls = {
            "overlapping views": lambda: _ffi.feather_paste(p(wide[..., :W]), p(wide[..., 8:]), e, B, H, W, 2, 3, stream()),
            "the same view twice": lambda: _ffi.feather_paste(p(dst), p(dst), e, B, H, W, 2, 3, stream()),
            "a row stride of 0 in dst": lambda: _ffi.feather_paste(p(src), (dst.data_ptr(), (dst.stride(0), dst.stride(1), 0, 1)), e, B, H, W, 2, 3, stream()),
            "an image stride of 0 in dst": lambda: _ffi.feather_paste(p(src), (dst.data_ptr(), (0,) + tuple(dst.stride()[1:])), e, B, H, W, 2, 3, stream()),
            "a negative ramp_y": lambda: _ffi.feather_paste(p(src), p(dst), e, B, H, W, -1, 3, stream()),
            "a negative ramp_x": lambda: _ffi.feather_paste(p(src), p(dst), e, B, H, W, 2, -3, stream()),
            "a ramp beyond 2^20": lambda: _ffi.feather_paste(p(src), p(dst), e, B, H, W, (1 << 20) + 1, 0, stream()),
            "an element code of 4": lambda: _ffi.feather_paste(p(src), p(dst), 4, B, H, W, 2, 3, stream()),
        }
        for what, call in calls.items():
            with pytest.raises(_ffi.MewZoomHipError) as err:
                call()
            assert err.value.code == _ffi.MZ_ERR_INVALID_ARGUMENT, what
            torch.cuda.synchronize()
            assert torch.equal(feather_ref.bits(dst), feather_ref.bits(before)) and torch.equal(feather_ref.bits(wide), feather_ref.bits(wide_before)), what
        with pytest.raises(TypeError):
            feather_paste(src, dst.float(), ramp=(2, 3))
        with pytest.raises(ValueError):
            feather_paste(src, dst[..., :-1], ramp=(2, 3))
        with pytest.raises(RuntimeError):
            feather_paste(src.cpu(), dst.cpu(), ramp=(2, 3))
        _ffi.feather_paste(p(src), p(dst), e, B, H, W, 1 << 20, 1 << 20, stream())  # the longest ramps are accepted
        torch.cuda.synchronize()
        assert same_bits(dst, feather_ref.paste_expected(src, before, (1 << 20, 1 << 20), dt))


# ---- upscale_feathered ---------------------------------------------------------------------------------------------------------------
def model_of(name, dt):
    return lower_built(name, torch.bfloat16 if dt == "u8" else DTYPES[dt])  # (a uint8 call runs the bf16 engine)


def image_of(Bx, H, W, dt, seed):
    x = synth_image(Bx, H, W, seed=seed)
    return (x * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).cuda() if dt == "u8" else x.to("cuda", DTYPES[dt])


def untiled(m, x):
    return m.upscale_uint8(x) if x.dtype == torch.uint8 else m.upscale(x)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_a_halo_of_receptive_field_plus_overlap_gives_the_bits_of_upscale(dt):
    m = model_of("g1", dt)  # g1_2x_c16
    x = image_of(2, 203, 277, dt, 13)  # odd sizes: floors and pads at every level; 4 x 3 tiles, ragged last row and column
    want = untiled(m, x)
    halo = receptive_field(m._cfg) + 16
    got = upscale_feathered(m, x, tile=(64, 120), halo=halo, overlap=16)
    assert same_bits(got, want)
    if dt == "bf16":  # once through the method, into a permuted HWC out
        hwc = torch.full((2, 406, 554, 3), 7.0, dtype=x.dtype, device="cuda")
        out = hwc.permute(0, 3, 1, 2)
        assert m.upscale_feathered(x, tile=(64, 120), halo=halo, overlap=16, out=out) is out
        assert same_bits(out.contiguous(), want)


def test_a_4x_model_in_the_exact_regime():
    m = model_of("g3", "f16")  # g3_4x_c16
    x = image_of(1, 171, 232, "f16", 14)
    got = upscale_feathered(m, x, tile=(80, 80), halo=receptive_field(m._cfg) + 16, overlap=16)
    assert same_bits(got, m.upscale(x))


SMALL = dict(H=67, W=109, tile=(24, 40), halo=8)  # 3 x 3 tiles, ragged last row and column, four-tile corners


def tiles_of(m, x, plan, r):
    """the kept result of every tile of a plan, each computed by upscale_into from the plan alone"""
    out = []
    for row in plan:
        out.append([])
        for t in row:
            s, k = t.slice, t.kept
            dst = torch.empty((x.shape[0], 3, (k.y1 - k.y0) * r, (k.x1 - k.x0) * r), dtype=x.dtype, device=x.device)
            m.upscale_into(x[:, :, s.y0 : s.y1, s.x0 : s.x1], dst, window=((k.y0 - s.y0) * r, (k.x0 - s.x0) * r, dst.shape[2], dst.shape[3]))
            out[-1].append(dst)
    return out


@functools.lru_cache(maxsize=None)
def small_case(dt, overlap):
    """(model, x, plan, the kept tiles on the CPU, the reference blend of them), computed once"""
    m = model_of("g1", dt)
    x = image_of(2, SMALL["H"], SMALL["W"], dt, 21)
    plan = plan_feathered(SMALL["H"], SMALL["W"], SMALL["tile"], SMALL["halo"], overlap)
    assert len(plan) == 3 and len(plan[0]) == 3
    tiles = [[t.cpu() for t in row] for row in tiles_of(m, x, plan, 2)]
    return m, x, plan, tiles, feather_ref.blend_expected(plan, tiles, 2, overlap, dt, 2, SMALL["H"], SMALL["W"])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_small_halo_tiles_are_blended_in_the_order_of_the_reference(dt):
    m, x, plan, tiles, want = small_case(dt, 4)
    got = upscale_feathered(m, x, tile=SMALL["tile"], halo=SMALL["halo"], overlap=4)
    assert same_bits(got, want)
    assert same_bits(upscale_feathered(m, x, tile=SMALL["tile"], halo=SMALL["halo"]), want)  # overlap defaults to halo // 2
    # overlap = 0 is the hard cut: every core as its tile gives it, nothing blended
    m, x, plan0, tiles0, want0 = small_case(dt, 0)
    hard = torch.empty_like(want0)
    for row, trow in zip(plan0, tiles0):
        for t, kept in zip(row, trow):
            hard[:, :, t.core.y0 * 2 : t.core.y1 * 2, t.core.x0 * 2 : t.core.x1 * 2] = kept
    assert same_bits(want0, hard)
    assert same_bits(upscale_feathered(m, x, tile=SMALL["tile"], halo=SMALL["halo"], overlap=0), hard)
    assert not same_bits(got, hard)


def test_the_feathered_result_lies_within_the_tiles_own_error():
    """f32.  eps = the largest deviation of any kept tile from upscale(x) on its kept window.  Every element of the result is a tile's
    element or comes from at most two convex combinations of tiles' elements (a row paste, then a strip paste), each rounded once to
    float32 on values in [0, 1] (half an ulp: at most 2^-25 each, and the second one's operand carries the first one's):
    max |feathered - upscale(x)| <= eps + 2^-22."""
    m, x, plan, tiles, want = small_case("f32", 4)
    full = m.upscale(x).cpu()
    eps = max(float((kept - full[:, :, t.kept.y0 * 2 : t.kept.y1 * 2, t.kept.x0 * 2 : t.kept.x1 * 2]).abs().max())
              for row, trow in zip(plan, tiles) for t, kept in zip(row, trow))
    got = upscale_feathered(m, x, tile=SMALL["tile"], halo=SMALL["halo"], overlap=4).cpu()
    err = float((got - full).abs().max())
    print(f"feathered f32, halo 8, overlap 4: eps {eps:.6e}, max |feathered - untiled| {err:.6e}")
    assert eps > 0.0  # (a halo of 8 is far below the receptive field: the tiles do deviate)
    assert err <= eps + 2.0 ** -22
    hard = upscale_feathered(m, x, tile=SMALL["tile"], halo=SMALL["halo"], overlap=0).cpu()
    band = (slice(None), slice(None), slice((24 - 4) * 2, (24 + 4) * 2), slice(None))  # the band around the cut at row 24
    assert not torch.equal(got[band], hard[band])
