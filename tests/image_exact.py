"""Exact-arithmetic reference of the filtering image operators (tests/test_image_exact_cpu.py, tests/test_image_exact_gpu.py): mz_interpolate's
bilinear and bicubic modes (mz_interp.h), mz_resize (mz_resize.h) and mz_blur (mz_degrade.h), restated in Python from the headers alone --
nothing here calls the library.  Needs no GPU.

  fma64            the correctly rounded float64 of a * b + c on numpy arrays: an error-free product and sum, the low parts added with
                   ROUNDING TO ODD (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", IEEE TC 2008), exact rational
                   arithmetic (fma_exact) wherever an intermediate of that scheme could leave the normal range
  *_taps           the tap tables, one IEEE operation of a Python float per operation of the header
  *_expected       the stored tensor: both passes as acc = fma(w_k, v_k, acc) in ascending k, the intermediate and the roundings as the header
                   of each operator states them.  `ar` swaps ONE statement for a plausible mistake (WRONG): the CPU test shows that the
                   cases below tell each of them from the reference
  CASES            the cases of the GPU test and their inputs, every one chosen from the reference alone"""

from __future__ import annotations

import math
from collections import namedtuple
from fractions import Fraction
from functools import lru_cache

import numpy as np
import torch

import degrade_ref
import exact_util
import interp_util
import resize_util
from resize_util import DTYPES

F64, F32 = np.float64, np.float32


# ---- fma ----------------------------------------------------------------------------------------------------------------------------------
def fma_exact(a: float, b: float, c: float) -> float:
    """One fma in rational arithmetic: int / int true division rounds correctly, subnormal results included"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return c if math.isfinite(a) and math.isfinite(b) else a * b + c  # no rounding is involved: IEEE's rules for infinities and NaN
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        return a * b + c  # a b is 0 or -c: exact as a float; the sum of two floats has the sign IEEE gives a zero
    try:
        return q.numerator / q.denominator
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_odd(a, b):
    """a + b rounded to odd: the nearest-even sum, moved to its odd neighbour on the side of the error when it is inexact and even"""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    step = np.where((e > 0) == (s > 0), 1, -1)  # the bit pattern grows away from zero
    return np.where((e != 0) & ((bits & 1) == 0), bits + step, bits).view(F64)


LO, HI = 2.0 ** -900, 2.0 ** 480


def fma64(a, b, c) -> np.ndarray:
    a, b, c = (np.ascontiguousarray(v, dtype=F64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        plain = a * b + c
        # a zero product is exact and c is added to it by IEEE's rules; to a nonzero product a zero c adds nothing: the product's rounding
        plain = np.where((c == 0) & (a != 0) & (b != 0), a * b, plain)
        plain = np.where(np.isfinite(a) & np.isfinite(b) & ~np.isfinite(c), c, plain)  # (a finite product that overflows is not an infinity)
        easy = ~(np.isfinite(a) & np.isfinite(b) & np.isfinite(c)) | (a == 0) | (b == 0) | (c == 0)
        pa, pb, pc, pp = np.abs(a), np.abs(b), np.abs(c), np.abs(a * b)
        inside = (pa < HI) & (pb < HI) & (pc < HI) & (pa > LO) & (pb > LO) & (pc > LO) & (pp > LO)
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        out = np.where(easy, plain, th + _add_odd(tl, ul))
    hard = ~easy & ~inside
    if hard.any():
        out = out.copy()
        out[hard] = [fma_exact(x, y, z) for x, y, z in zip(a[hard], b[hard], c[hard])]
    return out


# ---- the taps of one axis ---------------------------------------------------------------------------------------------------------------------
Taps = namedtuple("Taps", "idx w mask")  # [n_out, K] each: source index, weight, whether the tap exists


def _table(rows):
    K = max(len(r[0]) for r in rows)
    idx, w, mask = np.zeros((len(rows), K), dtype=np.int64), np.zeros((len(rows), K)), np.zeros((len(rows), K), dtype=bool)
    for i, (ii, ww) in enumerate(rows):
        idx[i, :len(ii)], w[i, :len(ww)], mask[i, :len(ii)] = ii, ww, True
    return Taps(idx, w, mask)


def interp_taps(n_in: int, n_out: int, mode: str, i: int):
    """mz_interp.h, THE TAPS: (indices, weights) of output index i"""
    if mode == "nearest":
        if n_in == n_out:
            return [i], [1.0]
        sf = F32(n_in) / F32(n_out)
        return [min(int(math.floor(F32(F32(i) * sf))), n_in - 1)], [1.0]
    s = float(n_in) / float(n_out)
    src = s * (float(i) + 0.5) - 0.5
    if mode == "bilinear":
        src = max(src, 0.0)
        i0 = min(int(src), n_in - 1)
        lam = src - float(i0)
        return [i0, i0 + (1 if i0 < n_in - 1 else 0)], [1.0 - lam, lam]
    A = -0.75
    f = math.floor(src)
    t = src - f
    idx = [min(max(int(f) - 1 + k, 0), n_in - 1) for k in range(4)]
    u0, u2, u3 = t + 1.0, 1.0 - t, 2.0 - t
    return idx, [((A * u0 - 5.0 * A) * u0 + 8.0 * A) * u0 - 4.0 * A, ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0,
                 ((A + 2.0) * u2 - (A + 3.0)) * u2 * u2 + 1.0, ((A * u3 - 5.0 * A) * u3 + 8.0 * A) * u3 - 4.0 * A]


def _resize_filter(filt: str, u: float) -> float:
    u = abs(u)
    if filt == "bilinear":
        return 1.0 - u if u < 1.0 else 0.0
    A = -0.5
    if u < 1.0:
        return ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0
    if u < 2.0:
        return (((u - 5.0) * u + 8.0) * u - 4.0) * A
    return 0.0


def resize_taps(n_in: int, n_out: int, filt: str, i: int):
    """mz_resize.h, resize_taps(): (first, weights)"""
    scale = float(n_in) / float(n_out)
    half = 1.0 if filt == "bilinear" else 2.0
    support = half * scale if scale >= 1.0 else half
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    center = scale * (float(i) + 0.5)
    lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)
    f = [_resize_filter(filt, (float(j + lo) - center + 0.5) * inv) for j in range(hi - lo)]
    total = 0.0
    for v in f:
        total += v
    return lo, [v / total for v in f]


def blur_weights(sigma: float):
    """mz_degrade.h, blur_weights()"""
    half = int(3.0 * sigma)
    w = [math.exp(-0.5 * ((float(j) / sigma) * (float(j) / sigma))) if half else math.exp(-0.5 * (0.0 * 0.0)) for j in range(-half, half + 1)]
    total = 0.0
    for v in w:
        total += v
    return [v / total for v in w]


def reflect(i: int, n: int) -> int:
    return -i if i < 0 else 2 * (n - 1) - i if i >= n else i


@lru_cache(maxsize=None)
def interp_table(n_in, n_out, mode) -> Taps:
    return _table([interp_taps(n_in, n_out, mode, i) for i in range(n_out)])


@lru_cache(maxsize=None)
def resize_table(n_in, n_out, filt) -> Taps:
    rows = [resize_taps(n_in, n_out, filt, i) for i in range(n_out)]
    return _table([(list(range(first, first + len(w))), w) for first, w in rows])


@lru_cache(maxsize=None)
def blur_table(n, sigma) -> Taps:
    w = blur_weights(sigma)
    half = len(w) // 2
    return _table([([reflect(i - half + j, n) for j in range(len(w))], w) for i in range(n)])


# ---- the arithmetic, and the mistakes it is told from ------------------------------------------------------------------------------------------
# acc: the accumulator's type; fused: acc = fma(w, v, acc), else a rounded product, then a rounded sum; descending: the taps in descending k;
# mid: the intermediate between the passes ("ref": as the header says, "storage": rounded to the stored type); final: the last rounding to the
# stored type ("rne"; "trunc": towards zero; "other_tie": ties away from zero for the float types, ties to even for uint8, whose rule is
# + 0.5 and truncate)
Arith = namedtuple("Arith", "acc fused descending mid final", defaults=("f64", True, False, "ref", "rne"))
REF = Arith()
WRONG = {"float32 accumulation": Arith(acc="f32"), "multiply, then add": Arith(fused=False), "descending taps": Arith(descending=True),
         "intermediate in the stored type": Arith(mid="storage"), "final truncation": Arith(final="trunc")}
OTHER_TIE = Arith(final="other_tie")


def accumulate(x: np.ndarray, t: Taps, ar: Arith) -> np.ndarray:
    """out[..., i] = sum_k w[i, k] x[..., idx[i, k]] along the last axis, from acc = +0 in the order and the arithmetic of `ar`"""
    order = range(t.w.shape[1] - 1, -1, -1) if ar.descending else range(t.w.shape[1])
    acc = np.zeros(x.shape[:-1] + (t.w.shape[0],), dtype=F32 if ar.acc == "f32" else F64)
    with np.errstate(all="ignore"):
        for k in order:
            v = x[..., t.idx[:, k]]
            if ar.acc == "f32":
                new = (t.w[:, k].astype(F32).astype(F64) * v.astype(F32).astype(F64) + acc.astype(F64)).astype(F32)
            elif ar.fused:
                new = fma64(t.w[:, k], v, acc)
            else:
                new = t.w[:, k] * v + acc
            acc = np.where(t.mask[:, k], new, acc)
    return acc.astype(F64)


def vertical(h: np.ndarray, t: Taps, ar: Arith) -> np.ndarray:
    return np.ascontiguousarray(accumulate(np.ascontiguousarray(h.swapaxes(-1, -2)), t, ar).swapaxes(-1, -2))


def clamp01(v: np.ndarray) -> np.ndarray:
    """fmin(fmax(v, 0), 1): a NaN becomes 0"""
    return np.fmin(np.fmax(v, 0.0), 1.0)


def round64(v: np.ndarray, dt: str, rule: str = "rne") -> torch.Tensor:
    """float64 -> the float type `dt` in ONE rounding (exact_util's integer arithmetic on the bit pattern); infinities and NaN pass"""
    a = np.ascontiguousarray(v, dtype=F64)
    fin = np.isfinite(a)
    out, _, tie, up = exact_util._round_parts(torch.from_numpy(np.where(fin, a, 0.0)), dt)
    if rule == "trunc":
        out = out - up
    elif rule == "other_tie":
        out = out + (tie & ~up)
    if dt == "f32":
        t = torch.from_numpy(out.astype(np.uint32).view(np.int32)).view(torch.float32).reshape(a.shape).clone()
    else:
        t = torch.from_numpy(out.astype(np.uint16).view(np.int16)).view(DTYPES[dt]).reshape(a.shape).clone()
    if not fin.all():
        t[torch.from_numpy(~fin)] = torch.from_numpy(a[~fin]).to(DTYPES[dt])
    return t


def u8_of_unit(f: np.ndarray, rule: str = "rne") -> np.ndarray:
    """mz_view.h in float32, the product and the sum rounded separately: clamp(v * 255 + 0.5, 0, 255), truncated"""
    f = f.astype(F32)
    with np.errstate(all="ignore"):
        t = f * F32(255.0)
        t = t if rule == "trunc" else np.rint(t) if rule == "other_tie" else t + F32(0.5)
        return np.fmin(np.fmax(t, F32(0.0)), F32(255.0)).astype(np.uint8)


def u8_of_unit_fused(f: np.ndarray) -> np.ndarray:
    """the same with ONE rounding of v * 255 + 0.5 to float32: the float64 product is exact (24 + 8 bits), and so is the float64 sum
    wherever it is not within 2^-20 of 0.5, where both forms truncate to 0"""
    t = (f.astype(F32).astype(F64) * 255.0 + 0.5).astype(F32)
    return np.fmin(np.fmax(t, F32(0.0)), F32(255.0)).astype(np.uint8)


def store_f32(f: np.ndarray, dt: str, clamp: int, rule: str) -> torch.Tensor:
    """st_f32 of mz_view.h on float32 values"""
    if dt == "u8":
        return torch.from_numpy(u8_of_unit(f, rule))
    if clamp:
        f = clamp01(f)
    return torch.from_numpy(f.astype(F32)) if dt == "f32" else round64(f.astype(F64), dt, rule)


def to_f32(v: np.ndarray, rule: str = "rne") -> np.ndarray:
    with np.errstate(all="ignore"):
        return v.astype(F32) if rule == "rne" else round64(v, "f32", rule).numpy()


Result = namedtuple("Result", "want last")  # the stored tensor; the value its last rounding sees (float64 array)


def interp_expected(x: torch.Tensor, size, mode: str, dt: str, clamp: int, window=None, ar: Arith = REF, detail: bool = False):
    """mz_interp.h, THE EVALUATION: float64 sums, a float64 intermediate, one rounding"""
    a = x.cpu()
    src = a.numpy().astype(F64) / 255.0 if dt == "u8" else a.double().numpy()
    h = accumulate(src, interp_table(a.shape[3], size[1], mode), ar)
    if ar.mid == "storage":
        h = finish64(h, dt, 0, "rne").double().numpy() / (255.0 if dt == "u8" else 1.0)
    v = vertical(h, interp_table(a.shape[2], size[0], mode), ar)
    if window is not None:
        y0, x0, hh, ww = window
        v = v[:, :, y0:y0 + hh, x0:x0 + ww]
    want = finish64(v, dt, clamp, ar.final)
    return Result(want, clamp01(v) if clamp or dt == "u8" else v) if detail else want


def finish64(v: np.ndarray, dt: str, clamp: int, rule: str) -> torch.Tensor:
    """interp_round_raw of mz_interp.hip"""
    with np.errstate(all="ignore"):
        if dt == "u8":
            t = clamp01(v) * 255.0
            t = t if rule == "trunc" else np.rint(t) if rule == "other_tie" else t + 0.5
            return torch.from_numpy(t.astype(np.uint8))
        if clamp:
            v = clamp01(v)
        return torch.from_numpy(v.astype(F32)) if (dt, rule) == ("f32", "rne") else round64(v, dt, rule)


def _two_pass_f32(a: torch.Tensor, tx: Taps, ty: Taps, dt: str, clamp: int, window, ar: Arith, detail: bool, once16: bool):
    """resize_kernel and blur_kernel: float32 source values, float64 sums, a float32 intermediate.  The second sum goes to the element
    through float32 -- (float)acc, then st_f32: clamp, the cast to a 16-bit type, or u8_of_unit -- except, with `once16` (st_f64, the
    blur), to a 16-bit type: the float64 sum rounded once."""
    a = a.cpu()
    src = (a.numpy().astype(F32) / F32(255.0)).astype(F64) if dt == "u8" else a.float().numpy().astype(F64)
    h = to_f32(accumulate(src, tx, ar))
    if ar.mid == "storage":
        s = store_f32(h, dt, 0, "rne")
        h = (s.numpy().astype(F32) / F32(255.0)) if dt == "u8" else s.float().numpy()
    v = vertical(h.astype(F64), ty, ar)
    if window is not None:
        y0, x0, hh, ww = window
        v = v[:, :, y0:y0 + hh, x0:x0 + ww]
    if once16 and dt in ("bf16", "f16"):
        want = round64(v, dt, ar.final)
        return Result(want, v) if detail else want
    f = to_f32(v, ar.final if dt == "f32" else "rne")
    want = store_f32(f, dt, clamp, ar.final)
    return Result(want, v if dt == "f32" else (clamp01(f) if clamp else f).astype(F64)) if detail else want


def resize_expected(x, size, filt: str, dt: str, clamp: int, window=None, ar: Arith = REF, detail: bool = False):
    return _two_pass_f32(x, resize_table(x.shape[3], size[1], filt), resize_table(x.shape[2], size[0], filt), dt, clamp, window, ar, detail, False)


def blur_expected(x, sigma: float, dt: str, ar: Arith = REF, detail: bool = False):
    """mz_degrade.h, BLUR: reflected indices, no clamp, a 16-bit result rounded once from the float64 sum.  k = 1 is the same two passes
    with the one weight 1.0: every value comes back, a -0 as +0 (fma(1, -0, +0))"""
    return _two_pass_f32(x, blur_table(x.shape[3], sigma), blur_table(x.shape[2], sigma), dt, 0, None, ar, detail, True)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """element-wise: equal bit patterns, or both NaN"""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    eq = interp_util.bits(got) == interp_util.bits(want)
    return eq if got.dtype == torch.uint8 else eq | (got.isnan() & want.isnan())


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
# op: interp / resize / blur; shape: ((Hin, Win), (Hout, Wout)), of blur (H, W); how: mode / filter / sigma; kind: the input (below);
# via: "" / "gather" (MZ_INTERP_GATHER) / "strided" (an output view with a column stride of 2: the element-store path) / "window"
Case = namedtuple("Case", "op shape how clamp kind via dts", defaults=(0, "noise", "", ("f32", "bf16", "f16", "u8")))
FLOATS = ("f32", "bf16", "f16")
B = 2
DYADIC_UP = ((9, 11), (18, 22))
RAGGED_UP, RAGGED_DOWN, UP3 = interp_util.RAGGED_UP, interp_util.RAGGED_DOWN, interp_util.UP3
RAGGED = resize_util.RAGGED  # 34 x 190 -> 17 x 95: exactly a half, the bilinear weights are 1/8, 3/8, 3/8, 1/8
INTERP_SHAPES = [DYADIC_UP, UP3, RAGGED_UP, RAGGED_DOWN, ((7, 5), (10, 13)), ((1, 1), (5, 7)), ((5, 7), (1, 1))]
RESIZE_SHAPES = [((37, 45), (12, 15)), ((48, 64), (36, 48)), UP3, ((17, 19), (2, 3)), resize_util.TAPS66, RAGGED, ((1, 7), (2, 3)), ((16, 16), (1, 1))]
BLUR_SHAPES = [(16, 16), (17, 33), (31, 15), (37, 45)]
BLUR_HALF15 = 5.0  # int(3 * 5.0) = 15 = kBlurMaxHalf
# number range: inputs (image - 0.5) 2^e, so that inputs and results are subnormals of the stored type: just below its smallest normal
# ("sub_hi") and a few units of its smallest subnormal ("sub_lo": most negative results round to -0).  bf16 has float32's exponents.
SUBNORMAL = {"sub_hi": {"f32": -127, "bf16": -127, "f16": -15}, "sub_lo": {"f32": -145, "bf16": -130, "f16": -20}}


def window_of(c: Case):
    """one window with an odd origin"""
    return (1, 3, c.shape[1][0] - 2, c.shape[1][1] - 4) if c.via == "window" else None


def _cases():
    cs = []
    for mode in ("bilinear", "bicubic"):
        cs += [Case("interp", s, mode, clamp) for s in INTERP_SHAPES for clamp in (0, 1)]
        cs += [Case("interp", RAGGED_UP, mode, 0, "noise", via) for via in ("gather", "strided", "window")]
        cs += [Case("interp", s, mode, 0, kind, "", FLOATS) for s in (RAGGED_UP, RAGGED_DOWN) for kind in ("sub_hi", "sub_lo")]
        cs += [Case("interp", DYADIC_UP, mode, 0, "ties"), Case("interp", DYADIC_UP, mode, 0, "nonfinite", "", FLOATS),
               Case("interp", UP3, mode, 0, "cancel", "", FLOATS)]
    cs += [Case("interp", s, "bicubic", 0, "over", "", ("f16",)) for s in (RAGGED_UP, RAGGED_DOWN)]
    for filt in ("bicubic", "bilinear"):
        cs += [Case("resize", s, filt) for s in RESIZE_SHAPES]
        cs += [Case("resize", RAGGED, filt, 1), Case("resize", RAGGED, filt, 0, "noise", "window")]
        cs += [Case("resize", s, filt, 0, kind, "", FLOATS) for s in (UP3, ((37, 45), (12, 15))) for kind in ("sub_hi", "sub_lo")]
        cs += [Case("resize", ((37, 45), (12, 15)), filt, 0, "nonfinite", "", FLOATS), Case("resize", ((48, 64), (36, 48)), filt, 0, "cancel", "", FLOATS)]
    # (shrinking to a third averages noise well below its maximum; at 3 / 4 the antialiased bicubic still overshoots)
    cs += [Case("resize", s, "bicubic", 0, "over", "", ("f16",)) for s in (UP3, ((48, 64), (36, 48)))]
    cs += [Case("resize", RAGGED, "bilinear", 0, "ties")]
    cs += [Case("blur", s, sigma) for s in BLUR_SHAPES for sigma in degrade_ref.BLUR_SIGMAS if int(3 * sigma) < min(s)]
    cs += [Case("blur", (37, 45), BLUR_HALF15)]
    # (a Gaussian's weights are positive and add up to 1: no overshoot, so no "over" case)
    cs += [Case("blur", (17, 33), sigma, 0, kind, "", FLOATS) for sigma in (0.2, 1.0) for kind in ("sub_hi", "sub_lo")]
    cs += [Case("blur", (17, 33), 1.0, 0, "nonfinite", "", FLOATS), Case("blur", (37, 45), 1.0, 0, "cancel", "", FLOATS)]
    return cs


def case_id(c: Case) -> str:
    shape = f"{c.shape[0]}x{c.shape[1]}" if c.op == "blur" else resize_util.shape_id(c.shape)
    return "-".join([c.op, shape, str(c.how)] + (["clamp"] if c.clamp else []) + ([c.kind] if c.kind != "noise" else []) + ([c.via] if c.via else []))


CASES = _cases()
PAIRS = [(c, dt) for c in CASES for dt in c.dts]


def pair_id(p) -> str:
    return f"{case_id(p[0])}-{p[1]}"


def in_shape(c: Case):
    return c.shape if c.op == "blur" else c.shape[0]


def one_by_one(c: Case) -> bool:
    return c.op != "blur" and (c.shape[0] == (1, 1) or c.shape[1] == (1, 1))


def horizontal_table(c: Case) -> Taps:
    if c.op == "blur":
        return blur_table(c.shape[1], c.how)
    return (interp_table if c.op == "interp" else resize_table)(c.shape[0][1], c.shape[1][1], c.how)


def expected(c: Case, dt: str, x: torch.Tensor, ar: Arith = REF, detail: bool = False):
    if c.op == "interp":
        return interp_expected(x, c.shape[1], c.how, dt, c.clamp, window_of(c), ar, detail)
    if c.op == "resize":
        return resize_expected(x, c.shape[1], c.how, dt, c.clamp, window_of(c), ar, detail)
    return blur_expected(x, c.how, dt, ar, detail)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def noise(c: Case, dt: str, seed: int) -> torch.Tensor:
    return (degrade_ref.image(B, *c.shape, dt, seed) if c.op == "blur" else resize_util.image(B, *c.shape[0], dt, seed)).clone()


TIE_UNIT = {"f32": 1 << 23, "bf16": 128, "f16": 1024, "u8": 0}  # the integers of [unit, 2 unit) are values of the type, one ulp apart


def ties_image(c: Case, dt: str, seed: int) -> torch.Tensor:
    """Integers of one binade (uint8: bytes) on a grid of `step` units, every fourth one moved by one unit up or down.  Channels 0 and 2
    are constant along y, channel 1 along x, so one pass reproduces its operand and the other one's dyadic weights (x2: sixteenths and
    two-hundred-fifty-sixths; a half: eighths) give results on and one input unit beside a rounding tie of the stored type."""
    H, W = in_shape(c)
    g = torch.Generator().manual_seed(seed)
    step = {"bilinear": 2, "bicubic": 16}[c.how] // (2 if dt == "u8" and c.how == "bilinear" else 1)
    unit = TIE_UNIT[dt]
    span = (unit if unit else 256) // step

    def line(n):
        v = unit + step * torch.randint(0, span, (B, n), generator=g)
        moved = v + torch.randint(-1, 2, (B, n), generator=g) * (torch.randint(0, 4, (B, n), generator=g) == 0)
        return moved.clamp(unit, (2 * unit if unit else 256) - 1)

    x = torch.stack([line(W)[:, None, :].expand(B, H, W), line(H)[:, :, None].expand(B, H, W), line(W)[:, None, :].expand(B, H, W)], dim=1)
    return x.to(torch.uint8) if dt == "u8" else x.double().to(DTYPES[dt])


def cancel_image(c: Case, dt: str, seed: int) -> torch.Tensor:
    """Signed noise in which, for as many output columns as have source columns of their own, the source column of the largest weight
    is replaced by what makes the horizontal sum cancel: -(sum of the other products) / that weight, rounded to the type.  What is left
    of such a sum is the rounding of that one input, 2^-24 of the products in float32, so an error of 2^-53 of a product -- a product
    rounded before it is added, another order -- is 2^-29 of the result and changes its float32 rounding in one element of some dozens."""
    t = horizontal_table(c)
    x = noise(c, "f32", seed).double() - 0.5
    used = set()
    for i in sorted(range(t.w.shape[0]), key=lambda i: (float(np.abs(t.w[i]).max()), i)):  # the most evenly weighted outputs first
        cols = [int(j) for j, m in zip(t.idx[i], t.mask[i]) if m]
        if len(cols) < 2 or len(set(cols)) < len(cols) or used & set(cols):
            continue
        used |= set(cols)
        k = int(np.argmax(np.abs(np.where(t.mask[i], t.w[i], 0.0))))
        rest = sum(float(t.w[i, j]) * x[..., cols[j]] for j in range(len(cols)) if j != k)
        x[..., cols[k]] = (-rest / float(t.w[i, k])).to(DTYPES[dt]).double()
    return x.to(DTYPES[dt])


def make_input(c: Case, dt: str, seed: int) -> torch.Tensor:
    if c.kind in ("noise",):
        return noise(c, dt, seed)
    if c.kind in SUBNORMAL:
        return ((noise(c, "f32", seed) - 0.5) * 2.0 ** SUBNORMAL[c.kind][dt]).to(DTYPES[dt])
    if c.kind == "over":  # 0 and the largest finite float16: what a bicubic adds beyond its inputs overflows
        return ((noise(c, "f32", seed) > 0.5).float() * 65504.0).to(DTYPES[dt])
    if c.kind == "ties":
        return ties_image(c, dt, seed)
    if c.kind == "cancel":
        return cancel_image(c, dt, seed)
    assert c.kind == "nonfinite", c.kind
    x = noise(c, dt, seed)
    H, W = in_shape(c)
    x[0, 0, H // 3, W // 2] = math.inf
    x[1, 1, H // 2, W // 3] = math.nan
    return x


def differs(c: Case, dt: str, x: torch.Tensor, ar: Arith, want: torch.Tensor) -> int:
    """elements in which the restatement `ar` departs from the reference's stored tensor"""
    return int((~same_bits(expected(c, dt, x, ar), want)).sum())


def applicable(c: Case, dt: str, name: str) -> bool:
    """resize and blur keep a float32 intermediate: with float32 storage "the intermediate in the stored type" IS the reference"""
    return not (name == "intermediate in the stored type" and dt == "f32" and c.op != "interp")


def tie_census(c: Case, dt: str, x: torch.Tensor):
    """(exact ties of the last rounding whose neighbour towards zero is even, the same with an odd one, elements within one input
    unit's share of a tie but not on it).  uint8: of the same operator on the bytes as numbers, which is exact: k + 1/2."""
    if dt == "u8":
        y = expected(c, "f32", x.float(), REF, True).last
        frac = y - np.floor(y)
        k = np.floor(y).astype(np.int64)
        tie = frac == 0.5
        return int((tie & (k % 2 == 0)).sum()), int((tie & (k % 2 == 1)).sum()), int(((np.abs(frac - 0.5) <= 0.25) & ~tie).sum())
    y = expected(c, dt, x, REF, True).last
    _, inexact, tie, up = exact_util._round_parts(torch.from_numpy(np.ascontiguousarray(y)), dt)
    return int((tie & ~up).sum()), int((tie & up).sum()), int((inexact & ~tie).sum())


MIN_TIES = 8  # of each parity, per planted case and type


@lru_cache(maxsize=None)
def case_seed(c: Case, dt: str) -> int:
    """The seed of a case's input, found from the reference alone (as interp_util.gate_seed): 7, or for a float32 "cancel" case the first
    seed of 7..38 whose input tells every applicable wrong restatement from the reference, for a planted case the first one with MIN_TIES
    exact ties of either parity."""
    if c.kind == "ties":
        for seed in range(7, 39):
            even, odd, _ = tie_census(c, dt, make_input(c, dt, seed))
            if min(even, odd) >= MIN_TIES:
                return seed
        raise AssertionError(f"no planted input for {case_id(c)} {dt}")
    if c.kind == "cancel" and dt == "f32":
        for seed in range(7, 39):
            x = make_input(c, dt, seed)
            want = expected(c, dt, x)
            if all(differs(c, dt, x, ar, want) > 0 for name, ar in WRONG.items() if applicable(c, dt, name)):
                return seed
        raise AssertionError(f"no input separates every wrong restatement for {case_id(c)}")
    return 7


@lru_cache(maxsize=None)
def case_input(c: Case, dt: str) -> torch.Tensor:
    """the case's input on the CPU, built once and left unchanged by its users"""
    return make_input(c, dt, case_seed(c, dt))


@lru_cache(maxsize=None)
def case_expected(c: Case, dt: str) -> Result:
    return expected(c, dt, case_input(c, dt), REF, True)
