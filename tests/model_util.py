"""Models the GPU model tests share (tests/test_model_gpu.py, tests/test_poison_forward_gpu.py): built once, never changed."""

import functools

from golden_util import GoldenCase
from oracle import mewzoom_oracle as oracle
from ultrazoom_amd import MewZoom
from ultrazoom_amd.synth import synth_image, synth_state_dict


def build(case_or_cfg, weights, dtype):
    cfg = case_or_cfg.config if isinstance(case_or_cfg, GoldenCase) else case_or_cfg
    m = MewZoom(**cfg)
    m.load_state_dict(weights)
    return m.to("cuda", dtype).eval()


# Channel counts chosen to reach every kernel variant: (primary channels, hidden ratio) -> fused mix on the 16x16x32 kernel
# with NT = 1, 2, 3 (C = 32, 64, 96), K that pads to 32-channel chunks with a half-zero last chunk (C = 80 -> conv2 K = 160),
# K that does not fit the 16x16x32 kernel (C = 24, 48 with hidden ratio 1 -> 32x32x16 kernels), two N tiles (hidden 4 x 48).
FUZZ_CONFIGS = [
    # ratio, channels (4 levels), layers, hidden ratio, (B, H, W)
    (2, (32, 64, 96, 128), (2, 2, 2, 2), 2, (2, 40, 72)),
    (2, (96, 96, 96, 96), (2, 2, 2, 2), 2, (1, 33, 47)),
    (2, (80, 48, 24, 16), (2, 2, 2, 2), 2, (1, 48, 64)),
    (4, (48, 24, 32, 64), (2, 2, 2, 2), 4, (1, 24, 40)),
    (2, (48, 96, 16, 32), (2, 3, 2, 2), 1, (3, 17, 29)),
    (2, (32, 64, 192, 192), (2, 2, 2, 2), 2, (2, 64, 104)),  # C = 192 levels: conv3r_kernel (96-channel N tiles)
]

LOWER_B = 24  # different images: the three statistics of lowp_gate_vs_matched need samples (2X, 8 x 8: 18 432 output elements)


def _config(r, ch, layers, hr):
    cfg = {"upscale_ratio": r, "hidden_ratio": hr, "num_deg_features": 3}
    for n, c, l in zip(("primary", "secondary", "tertiary", "quaternary"), ch, layers):
        cfg[f"{n}_channels"] = c
        cfg[f"{n}_layers"] = l
    return cfg


# a thin, wide 2X model (76 M parameters): conv3r, mix16b (C = 192) and mix16 (C = 384, 768) on the 4 x 4, 2 x 2 and 1 x 1 levels
WIDE_CONFIG = _config(2, (96, 192, 384, 768), (2, 2, 2, 2), 2)
LOWER_MODELS = {
    "g1": "g1_2x_c16", "g3": "g3_4x_c16", "g4": "g4_8x_c16", "g8": "g8_c24_f5",  # 2X, 4X, 8X; pad channels
    "g7": "g7_cfg1_2x_c48",                                                       # 48 channels: conv3t, conv3r_ragged
    "c96": next(_config(r, ch, l, hr) for r, ch, l, hr, _ in FUZZ_CONFIGS if ch == (96, 96, 96, 96)),
    "wide": WIDE_CONFIG,
}


@functools.lru_cache(maxsize=None)
def lower_model(name):
    """(config, state dict) of a model of LOWER_MODELS: a fixture's own weights, or hash-initialised ones."""
    spec = LOWER_MODELS[name]
    if isinstance(spec, str):
        case = GoldenCase(spec)
        return case.config, case.weights()
    return spec, synth_state_dict(oracle.parameter_shapes(spec), seed=sum(ord(c) for c in name))


@functools.lru_cache(maxsize=None)
def lower_built(name, dtype):
    cfg, sd = lower_model(name)
    return build(cfg, sd, dtype)


def lower_image(H, W, B=LOWER_B):
    return synth_image(B, H, W, seed=1000 * H + W)
