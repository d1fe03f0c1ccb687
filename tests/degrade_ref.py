"""CPU checkers of the degradation kernels (ultrazoom_amd/csrc/mz_degrade.h): independent restatements in torch float64 and numpy.

  blur_ref     torch float64: F.pad(reflect) + conv2d, one axis after the other, weights exp(-0.5 (j / sigma)^2) / sum
  philox       Philox4x32-10 on numpy uint32 / uint64 arrays, from the published algorithm (Salmon et al., SC'11)
  noise_ref    Box-Muller on its first two words, float64; clamp(x + sigma n, 0, 1)
  jpeg_ref     the JPEG model of the header, numpy int64 / float64; jpeg_near_tie: the blocks (and the pixels they feed) in which a
               coefficient's c / Q lies within 1e-6 of a half, where a float64 sum in another order may round the other way
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance)
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
               103, 99], dtype=np.int64).reshape(8, 8)
K2 = np.full((8, 8), 99, dtype=np.int64)
K2[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def as_double(x: torch.Tensor) -> torch.Tensor:
    x = x.cpu()
    return x.double() / 255 if x.dtype == torch.uint8 else x.double()


# ---- blur --------------------------------------------------------------------------------------------------------------------------------
def blur_weights(sigma: float) -> torch.Tensor:
    half = int(3 * sigma)
    j = torch.arange(-half, half + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * (j / sigma) ** 2) if half else torch.ones(1, dtype=torch.float64)
    return w / w.sum()


def blur_ref(x: torch.Tensor, sigma: float) -> torch.Tensor:
    """float64 [B, 3, H, W] of a tensor of any element type"""
    z = as_double(x)
    w = blur_weights(sigma)
    half = (len(w) - 1) // 2
    if half == 0:
        return z
    C = z.shape[1]
    z = F.pad(z, (half, half, half, half), mode="reflect")
    z = F.conv2d(z, w.view(1, 1, 1, -1).expand(C, 1, 1, -1).contiguous(), groups=C)
    return F.conv2d(z, w.view(1, 1, -1, 1).expand(C, 1, -1, 1).contiguous(), groups=C)


# ---- noise -------------------------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of uint32 words (broadcast against each other); returns the four output words"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def normal_ref(n: int, seed: int, stream: int) -> np.ndarray:
    """n of elements 0 .. n - 1 of stream `stream` of `seed`, float64"""
    i = np.arange(n, dtype=np.uint64)
    stream &= 2**64 - 1
    u = philox(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1 = (u[0].astype(np.float64) + 0.5) / 4294967296.0
    u2 = (u[1].astype(np.float64) + 0.5) / 4294967296.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise_ref(x: torch.Tensor, sigma: float, seed: int, offset: int = 0) -> torch.Tensor:
    """float64 [B, 3, H, W]: clamp(x + sigma n, 0, 1), image b from stream offset + b"""
    z = as_double(x)
    B = z.shape[0]
    n = np.stack([normal_ref(z[0].numel(), seed, offset + b).reshape(z.shape[1:]) for b in range(B)])
    return (z + sigma * torch.from_numpy(n)).clamp(0, 1)


# ---- JPEG --------------------------------------------------------------------------------------------------------------------------------
def qtables(quality: int):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (K1, K2))


def dct_matrix() -> np.ndarray:
    """T[u][x] of the orthonormal 8-point DCT-II"""
    x = np.arange(8, dtype=np.float64)
    T = np.stack([0.5 * np.cos((2 * x + 1) * u * (np.pi / 16)) for u in range(8)])
    T[0] = np.sqrt(0.125)
    return T


S4 = np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.int64)
SIGN = {0: np.ones(8, dtype=np.int64), 4: S4}
EXACT = np.zeros((8, 8), dtype=bool)
EXACT[np.ix_([0, 4], [0, 4])] = True


def to_8bit(x: torch.Tensor) -> np.ndarray:
    """step 1: int64 [B, 3, H, W]"""
    x = x.cpu()
    if x.dtype == torch.uint8:
        return x.numpy().astype(np.int64)
    v = x.float().numpy().astype(np.float32) * np.float32(255.0) + np.float32(0.5)
    return np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0).astype(np.uint8).astype(np.int64)


def _blocks(p: np.ndarray) -> np.ndarray:
    """[H, W] -> [H / 8, W / 8, 8, 8]"""
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b: np.ndarray) -> np.ndarray:
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def code_plane(p: np.ndarray, Q: np.ndarray):
    """steps 5-8 of one padded plane (int64 samples 0..255): (decoded plane, near-tie flag per block [H / 8, W / 8])"""
    T = dct_matrix()
    f = _blocks(p - 128)                                    # [.., y, x]
    C = np.einsum("vy,ux,nmyx->nmvu", T, T, f.astype(np.float64), optimize=False)
    ratio = np.abs(C) / Q
    level = np.sign(C) * np.floor(ratio + 0.5)
    frac = ratio - np.floor(ratio)
    near = (np.abs(frac - 0.5) <= 1e-6) & ~EXACT
    level = level.astype(np.int64)
    for v in (0, 4):
        for u in (0, 4):
            S = np.einsum("y,x,nmyx->nm", SIGN[v], SIGN[u], f)
            level[..., v, u] = np.sign(S) * ((np.abs(S) + 4 * Q[v, u]) // (8 * Q[v, u]))
    D = level * Q
    R = np.einsum("vy,ux,nmvu->nmyx", T, T, np.where(EXACT, 0, D).astype(np.float64), optimize=False)
    E = np.zeros_like(D)
    for v in (0, 4):
        for u in (0, 4):
            E = E + SIGN[v][:, None] * SIGN[u][None, :] * D[..., v, u][..., None, None]
    val = np.floor((E + 1024) / 8.0 + R + 0.5)
    return _unblocks(np.clip(val, 0, 255).astype(np.int64)), near.any(axis=(2, 3))


def _upsample(P: np.ndarray, H: int, W: int) -> np.ndarray:
    """step 9: chroma plane [ceil(H / 2), ceil(W / 2)] -> [H, W]"""
    ch, cw = P.shape
    y, x = np.arange(H), np.arange(W)
    ny, nx = y // 2, x // 2
    fy = np.clip(np.where(y & 1, ny + 1, ny - 1), 0, ch - 1)
    fx = np.clip(np.where(x & 1, nx + 1, nx - 1), 0, cw - 1)
    col = 3 * P[ny] + P[fy]                                  # [H, cw]
    return (3 * col[:, nx] + col[:, fx] + np.where(x & 1, 7, 8)[None, :]) >> 4


def _spread(flag: np.ndarray, H: int, W: int, chroma: bool) -> np.ndarray:
    """pixels [H, W] that a flagged block feeds: its own 8 x 8 (luminance) or 16 x 16 plus one pixel around (chroma, through step 9)"""
    size = 16 if chroma else 8
    m = np.kron(flag.astype(np.uint8), np.ones((size, size), dtype=np.uint8)).astype(bool)
    if chroma:
        g = m.copy()
        g[1:] |= m[:-1]; g[:-1] |= m[1:]
        m = g.copy()
        m[:, 1:] |= g[:, :-1]; m[:, :-1] |= g[:, 1:]
    return m[:H, :W]


def jpeg_ref(x: torch.Tensor, quality: int):
    """The model of mz_degrade.h on a [B, 3, H, W] tensor: (uint8 result [B, 3, H, W] as int64 numpy, pixels fed by a near-tie block
    [B, H, W] bool, share of near-tie blocks)"""
    rgb = to_8bit(x)
    B, _, H, W = rgb.shape
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    QY, QC = qtables(quality)
    out = np.zeros_like(rgb)
    unsure = np.zeros((B, H, W), dtype=bool)
    flagged = total = 0
    for b in range(B):
        r, g, bl = rgb[b]
        planes = [np.clip((299 * r + 587 * g + 114 * bl + 500) // 1000, 0, 255),
                  np.clip((-168736 * r - 331264 * g + 500000 * bl + 128500000) // 1000000, 0, 255),
                  np.clip((500000 * r - 418688 * g - 81312 * bl + 128500000) // 1000000, 0, 255)]
        planes = [np.pad(p, ((0, Hp - H), (0, Wp - W)), mode="edge") for p in planes]
        bias = np.tile(np.array([1, 2], dtype=np.int64), Wp // 4)[None, :]
        for k in (1, 2):
            p = planes[k]
            planes[k] = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        dec, flags = zip(*(code_plane(p, QY if k == 0 else QC) for k, p in enumerate(planes)))
        flagged += sum(int(f.sum()) for f in flags)
        total += sum(f.size for f in flags)
        yv = dec[0][:H, :W]
        db = _upsample(dec[1][:(H + 1) // 2, :(W + 1) // 2], H, W) - 128
        dr = _upsample(dec[2][:(H + 1) // 2, :(W + 1) // 2], H, W) - 128
        out[b, 0] = np.clip((1000000 * yv + 1402000 * dr + 500000) // 1000000, 0, 255)
        out[b, 1] = np.clip((1000000 * yv - 344136 * db - 714136 * dr + 500000) // 1000000, 0, 255)
        out[b, 2] = np.clip((1000000 * yv + 1772000 * db + 500000) // 1000000, 0, 255)
        unsure[b] = _spread(flags[0], H, W, False) | _spread(flags[1], H, W, True) | _spread(flags[2], H, W, True)
    return out, unsure, flagged / total


def jpeg_expected(x: torch.Tensor, quality: int, dtype: torch.dtype):
    """(expected tensor of `dtype`, unsure pixels [B, 1, H, W] bool tensor, share of near-tie blocks): a float element holds the 8-bit
    result / 255 rounded once to the type (tests/test_degrade_cpu.py shows float32's quotient rounds to the same 16-bit value)"""
    out, unsure, share = jpeg_ref(x, quality)
    t = torch.from_numpy(out)
    want = t.to(torch.uint8) if dtype == torch.uint8 else (t.float() / 255.0).to(dtype)
    return want, torch.from_numpy(unsure)[:, None], share


# ---- the cases of tests/test_degrade_gpu.py, shared with tests/test_degrade_cpu.py and tests/test_poison_degrade_gpu.py ---------------------
SHAPES = [(16, 16), (17, 33), (31, 15), (37, 45), (64, 80)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.uint8}
ELEM = {"f32": 0, "bf16": 1, "f16": 2, "u8": 3}
BLUR_SIGMAS = (0.2, 0.34, 1.0, 2.5)
NOISE_SIGMAS = (0.05, 0.3)
QUALITIES = (20, 50, 90, 100)
BATCH, SEED, OFFSET = 3, 1234, 5


def shape_id(s):
    return f"{s[0]}x{s[1]}"


@lru_cache(maxsize=None)
def image(B: int, H: int, W: int, dt: str, seed: int = 21) -> torch.Tensor:
    """uniform noise in [0, 1], rounded to the element type, on the CPU"""
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed + 1000 * B + H * W), dtype=torch.float32)
    return (x * 255.0).round().to(torch.uint8) if dt == "u8" else x.to(DTYPES[dt])


def hip():
    from ultrazoom_amd import degrade

    return degrade
