"""mz_forward, mz_forward_u8 and mz_forward_view on a dirty workspace, through the handle, every pointer carved from an Arena
(tests/poison_util.py).

mz_forward never clears its workspace: pad channels, the zero border of an odd-sized sub-pixel target and the floors of PixelCrush are
right only if some kernel of the SAME call wrote them before another read them.  So the workspace starts as zeros (the baseline), as
0xFF bytes (NaN in every float type) and as 0x7F bytes (0x7F7F7F7F: a huge finite value as bf16 and f32, NaN as f16, so that a
min / max which drops NaN cannot hide the read); x sits between NaN guards, sr, qa and the workspace between pattern guards.  sr and qa
must have the baseline's bits and be finite, and no guard and no input may change."""

import functools

import pytest
import torch

from golden_util import GoldenCase
from model_util import FUZZ_CONFIGS, lower_built, lower_image
from poison_util import Arena, room
from ultrazoom_amd import MewZoom
from ultrazoom_amd.synth import synth_image, synth_state_dict

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
WORKSPACE_FILLS = (0x00, 0xFF, 0x7F)  # the baseline first
C96 = "c96"  # the hash-initialised 96-channel model of FUZZ_CONFIGS: conv2 + mix of every block on conv3r_kernel's fused variant


def c96_config():
    r, ch, layers, hr, shape = next(s for s in FUZZ_CONFIGS if s[1] == (96, 96, 96, 96))
    cfg = {"upscale_ratio": r, "hidden_ratio": hr, "num_deg_features": 3}
    for n, c, l in zip(("primary", "secondary", "tertiary", "quaternary"), ch, layers):
        cfg[f"{n}_channels"] = c
        cfg[f"{n}_layers"] = l
    return cfg, shape


@functools.lru_cache(maxsize=None)
def model_and_image(name: str, dt: str):
    """(the model, its engine, a float32 CPU image [B, 3, H, W]): built once per model and dtype"""
    if name == C96:
        from oracle import mewzoom_oracle as oracle

        cfg, (B, H, W) = c96_config()
        sd, x = synth_state_dict(oracle.parameter_shapes(cfg), seed=96), synth_image(B, H, W, seed=H * W)
    else:
        case = GoldenCase(name)
        cfg, sd, x = case.config, case.weights(), case.image()
    m = MewZoom(**cfg)
    m.load_state_dict(sd)
    m = m.to("cuda", DTYPES[dt]).eval()
    return m, m._get_engine(torch.empty(0, dtype=DTYPES[dt], device="cuda")), x


def nbytes(shape, dtype):
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= s
    return n


def run_fills(arena, ws, outputs, call):
    """`call()` once per workspace fill, the outputs refilled each time: every run has the bits of the first and leaves the arena intact."""
    base = None
    for fill in WORKSPACE_FILLS:
        ws.fill_(fill)
        for o in outputs:
            o.fill_(5 if o.dtype == torch.uint8 else -3.0)
        call()
        arena.check()
        got = [o.clone() for o in outputs]
        for g in got:
            if g.dtype != torch.uint8:
                assert bool(torch.isfinite(g.float()).all()), f"workspace of 0x{fill:02x} bytes: a result is not finite"
        if base is None:
            base = got
        for g, b in zip(got, base):
            assert torch.equal(g, b), f"workspace of 0x{fill:02x} bytes: the result differs from the zero-filled workspace's"
    return base


MODELS = [
    ("g1_2x_c16", ("f32", "bf16")),
    ("g2_odd_37x45", ("f32", "bf16", "f16")),  # levels 18 x 22, 9 x 11, 4 x 5: every floor and every zero border
    ("g8_c24_f5", ("f32", "bf16")),            # pad channels at every level
    ("g3_4x_c16", ("f32", "bf16")),            # two heads
    ("g7_cfg1_2x_c48", ("f32", "bf16")),       # conv3t_kernel
    (C96, ("f32", "bf16", "f16")),
]


# the smallest images (test_model_gpu.LOWER_MODELS): 8 x 8 has a 1 x 1 level 4; at 15 x 15 (7 x 7, 3 x 3, 1 x 1) every level has a floor
# and every up-conv a zero border that is larger than the data
LOWER = [
    ("g1", ("f32", "bf16")),
    ("g8", ("f32", "bf16")),          # pad channels at every level
    ("g7", ("f32", "bf16")),          # conv3t_kernel, conv3r's ragged variant
    ("c96", ("f32", "bf16", "f16")),  # conv3r_kernel and its fused variant
    ("wide", ("f32", "bf16", "f16")),  # mix16b, mix16
]
LOWER_SIZES = [(8, 8), (15, 15)]


@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("name,dt", [(n, dt) for n, dts in MODELS for dt in dts])
def test_forward_does_not_depend_on_the_workspace_s_contents(name, dt, clamp):
    m, engine, x = model_and_image(name, dt)
    check_forward(m, engine, x, dt, clamp)


@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("size", LOWER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name,dt", [(n, dt) for n, dts in LOWER for dt in dts])
def test_forward_of_the_smallest_images_does_not_depend_on_the_workspace_s_contents(name, dt, size, clamp):
    m = lower_built(name, DTYPES[dt])
    check_forward(m, m._get_engine(torch.empty(0, dtype=DTYPES[dt], device="cuda")), lower_image(*size, B=3), dt, clamp)


def check_forward(m, engine, x, dt, clamp):
    dtype = DTYPES[dt]
    B, _, H, W = x.shape
    r, F = engine.config["upscale_ratio"], engine.config["num_deg_features"]
    need = engine.handle.workspace_bytes(B, H, W, 0)
    sr_shape = (B, 3, r * H, r * W)
    arena = Arena("cuda", room(nbytes(x.shape, dtype), nbytes(sr_shape, dtype), 4 * B * F, need))
    xd = arena.input(x.to("cuda", dtype), name="x")
    sr = arena.output(sr_shape, dtype, name="sr")
    qa = arena.output((B, F), torch.float32, name="qa")
    ws = arena.raw(need, 0, name="workspace")
    stream = torch.cuda.current_stream().cuda_stream
    base_sr, base_qa = run_fills(arena, ws, [sr, qa], lambda: engine.handle.forward(
        xd.data_ptr(), sr.data_ptr(), qa.data_ptr(), B, H, W, clamp, ws.data_ptr(), need, 0, stream))
    # the arena changes addresses only: the module's own call (its own workspace, fresh tensors) gives the same bits
    want_sr, want_qa = m.forward(x.to("cuda", dtype))
    if clamp:
        want_sr = m.upscale(x.to("cuda", dtype))
    assert torch.equal(base_sr, want_sr) and torch.equal(base_qa.to(dtype), want_qa)


def test_the_second_micro_batch_runs_on_what_the_first_left_behind():
    """B = 3 in micro-batches of two: images 0, 1 and then image 2 through ONE workspace."""
    m, engine, _ = model_and_image("g2_odd_37x45", "bf16")
    B, H, W, dtype = 3, 37, 45, torch.bfloat16
    x = synth_image(B, H, W, seed=7)
    r, F = engine.config["upscale_ratio"], engine.config["num_deg_features"]
    need = engine.handle.workspace_bytes(B, H, W, 2)
    assert need < engine.handle.workspace_bytes(B, H, W, 3)
    sr_shape = (B, 3, r * H, r * W)
    arena = Arena("cuda", room(nbytes(x.shape, dtype), nbytes(sr_shape, dtype), 4 * B * F, need))
    xd = arena.input(x.to("cuda", dtype), name="x")
    sr = arena.output(sr_shape, dtype, name="sr")
    qa = arena.output((B, F), torch.float32, name="qa")
    ws = arena.raw(need, 0, name="workspace")
    stream = torch.cuda.current_stream().cuda_stream
    base_sr, base_qa = run_fills(arena, ws, [sr, qa], lambda: engine.handle.forward(
        xd.data_ptr(), sr.data_ptr(), qa.data_ptr(), B, H, W, 0, ws.data_ptr(), need, 2, stream))
    for b in range(B):  # and every image is what it is alone
        alone_sr, alone_qa = m.forward(x[b : b + 1].to("cuda", dtype))
        assert torch.equal(base_sr[b : b + 1], alone_sr) and torch.equal(base_qa[b : b + 1].to(dtype), alone_qa), b


@pytest.mark.parametrize("guard", [0xFF, 0x00])
def test_forward_u8(guard):
    """uint8 images have no NaN: the guards around x are 0xFF and then 0x00 bytes, and the result may depend on neither."""
    m, engine, _ = model_and_image("g1_2x_c16", "bf16")
    B, H, W = 2, 37, 45
    x = (synth_image(B, H, W, seed=41) * 255.0).round().to(torch.uint8)
    r = engine.config["upscale_ratio"]
    need = engine.handle.workspace_bytes(B, H, W, 0)
    sr_shape = (B, 3, r * H, r * W)
    arena = Arena("cuda", room(x.numel(), nbytes(sr_shape, torch.uint8), need))
    xd = arena.input(x.cuda(), name="x", fill=guard)
    sr = arena.output(sr_shape, torch.uint8, fill=5, name="sr")
    ws = arena.raw(need, 0, name="workspace")
    stream = torch.cuda.current_stream().cuda_stream
    (base,) = run_fills(arena, ws, [sr], lambda: engine.handle.forward_u8(xd.data_ptr(), sr.data_ptr(), 0, B, H, W, ws.data_ptr(), need, 0, stream))
    assert torch.equal(base, m.upscale_uint8(x.cuda()))


@pytest.mark.parametrize("kind,frame", [("bf16", 0xFF), ("f32", 0xFF), ("u8", 0xFF), ("u8", 0x00)])
def test_forward_view_of_a_crop_inside_a_poisoned_frame_into_a_window(kind, frame):
    """x is a crop of a larger image whose other pixels are NaN (uint8: 0xFF, then 0x00); the output is a window of the result inside
    a larger tensor whose other elements must keep their value."""
    m, engine, _ = model_and_image("g1_2x_c16", "bf16" if kind == "u8" else kind)
    dtype = torch.uint8 if kind == "u8" else DTYPES[kind]
    B, H, W, top, left = 2, 37, 45, 3, 5
    x = synth_image(B, H, W, seed=41)
    x = (x * 255.0).round().to(torch.uint8) if kind == "u8" else x.to(dtype)
    r = engine.config["upscale_ratio"]
    window = (3, 5, r * H - 7, r * W - 6)  # y0, x0, h, w in output pixels
    big_in = torch.full((B, 3, H + top + 6, (W + left + 6) * x.element_size()), frame, dtype=torch.uint8).view(dtype)
    assert big_in.shape == (B, 3, H + top + 6, W + left + 6) and (kind == "u8" or bool(torch.isnan(big_in.float()).all()))
    big_in[:, :, top : top + H, left : left + W] = x
    out_shape = (B, 3, window[2] + 2 + 5, window[3] + 3 + 7)
    need = engine.handle.workspace_bytes(B, H, W, 0)
    arena = Arena("cuda", room(nbytes(big_in.shape, dtype), nbytes(out_shape, dtype), need))
    bd = arena.input(big_in.cuda(), name="x frame", fill=frame)
    xv = bd[:, :, top : top + H, left : left + W]
    big_out = arena.output(out_shape, dtype, name="out frame")
    ov = big_out[:, :, 2 : 2 + window[2], 3 : 3 + window[3]]
    mask = torch.zeros(out_shape, dtype=torch.bool, device="cuda")
    mask[:, :, 2 : 2 + window[2], 3 : 3 + window[3]] = True
    ws = arena.raw(need, 0, name="workspace")
    stream = torch.cuda.current_stream().cuda_stream
    sentinel = 5 if kind == "u8" else -3.0  # what run_fills puts into the outputs before each call

    def call():
        engine.handle.forward_view(xv.data_ptr(), xv.stride(), ov.data_ptr(), ov.stride(), 0, B, H, W, True, 1 if kind == "u8" else 0, window,
                                   ws.data_ptr(), need, 0, stream)
        torch.cuda.synchronize()
        assert bool((big_out[~mask] == sentinel).all()), "an element outside the output window was written"

    (base,) = run_fills(arena, ws, [big_out], call)
    dense = m.upscale_uint8(x.cuda()) if kind == "u8" else m.upscale(x.cuda())
    assert torch.equal(base[:, :, 2 : 2 + window[2], 3 : 3 + window[3]], dense[:, :, 3 : 3 + window[2], 5 : 5 + window[3]])
