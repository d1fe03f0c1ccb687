"""Exact-arithmetic test data (tests/test_exact_cpu.py, tests/test_exact_gpu.py).  Needs no GPU.

Integer-valued activations and weights whose partial sums stay below 2^24 are added without error in fp32 in ANY order, so a kernel's
output must equal the float64 result rounded ONCE to the storage type, bit for bit, whatever its tile walk or K order.  This module
draws, for every row of the table below, the inputs; finish() adds what follows from the entry's one statement in tests/op_ref.py: the
float64 reference (torch.nn.functional on float64, the crop / zero border and the pixel shuffle from oracle.mewzoom_oracle), and with
it the expected storage-type tensor (round_once) and the figures the CPU test holds every
row to (absolute-product sums, maxima, the census of roundings and ties, the excluded share).

Where an operator contains a transcendental (the sigmoid of the mix's gate; SiLU in the one family that exists only with SiLU), the
data SATURATE it: for an argument t >= SAT_HI, e^-t < 2^-46 vanishes beside 1 in fp32 and the sigmoid is exactly 1; for t <= SAT_LO,
e^-t overflows fp32 and the sigmoid is exactly 0.  Elements in between are excluded from the equality (at most MAX_EXCLUDED of a row)
and compared with the one-operator tolerance instead."""

from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from gpu_util import DTYPES
import op_ref
from op_cases import CASES, TINY_CASES, fields

SAT_HI, SAT_LO = 32.0, -100.0
MAX_EXCLUDED = 0.02
MIN_BRANCH = 0.30
EXACT_SUM = float(2 ** 24)  # integers below it are fp32 values; a sum of absolute products below it bounds every partial sum
F16_MAX_OUT = 32768.0
AW = 7            # 3x3 / 2x2 weights: integers in [-AW, AW]
GATE_SCALE = 16   # gate weights: integers times 16 (exact in bf16 and f16); the gate then leaves (SAT_LO, SAT_HI) almost everywhere
# the largest integer magnitude below which EVERY integer is a value of the type (activations must be stored exactly)
INT_MAX = {"f32": 2047, "bf16": 255, "f16": 2047}
# f16 rounds integers only from 2048 on: rows of that type (and the SiLU row, whose window (SAT_LO, SAT_HI) must be a small share of
# the output's spread) get activations large enough for an output standard deviation of about SIGMA; |max| stays below 32768 = 9 SIGMA
SIGMA = 3600.0

# (entry, arguments, environment knobs, dtype, expected mz_debug_last_kernel() or None, silu)
Row = namedtuple("Row", "entry args env dt kernel silu")
PERSISTENT = {"conv3p", "conv3s", "conv3s_fused", "conv3r", "conv3r_8x40", "conv3r_ragged", "conv3r_fused", "conv3t", "conv3t_fused", "mix16b"}


def _rows():
    """tests/op_cases.CASES (the smallest shapes at which each family is chosen, pinned by the MZ_* knobs), conv and film
    with silu = 0 -- SiLU is not exact --, plus two shapes of this table's own.  conv3r's ragged variant exists only as conv1 + SiLU
    (choose_conv3, mz_select.h): its rows keep SiLU, on data that saturate it, and run once more without, on whatever family the host
    then chooses."""
    rows = []
    for entry, args, env, dt, kernel in CASES:
        if entry in ("conv", "film"):
            if kernel == "conv3r_ragged":
                rows.append(Row(entry, tuple(args[:5]) + (1,), env, dt, kernel, 1))
                kernel = "conv3w"  # without SiLU: Cin = 48 pads a third of a second 32-channel chunk, too much for the 16x16x32 kernels
            args = tuple(args[:5]) + (0,)
        rows.append(Row(entry, tuple(args), env, dt, kernel, 0))
    for dt in ("f32", "bf16", "f16"):
        # Cin = 144: the last 32-channel chunk of the 16x16x32 kernels is half zero planes (the f32 row has no such chunk)
        rows.append(Row("conv", (1, 20, 130, 144, 96, 0), {}, dt, "conv3w" if dt == "f32" else "conv3s", 0))
        rows.append(Row("conv", (1, 5, 9, 160, 16, 0), {}, dt, "conv3w" if dt == "f32" else "conv3s", 0))
    seen = {}
    for r in rows:
        seen.setdefault(row_id(r), r)
    return list(seen.values())


# The rows of the lower edge (TINY_CASES: 1 x 1, one row, one column, 2 x 3) are there for their geometry.  The census of roundings and ties
# that tests/test_exact_cpu.py asks of a row needs at least 100 exact ties at a share of at least 0.01: 10 000 elements at that floor.  A
# lower-edge row with fewer compared elements (48 to a few thousand) is held to the share that needs rounding where it has at least
# CENSUS_MIN_SHARE elements (0.01 of them are then ten), and its family's ties are pinned by a row of ordinary size of the same entry,
# family and type, which the CPU test checks exists.  Every other condition (exact sums, exact inputs, the f16 range, the excluded share,
# both saturated branches) holds for these rows as for any other.  Rows are named one by one: an ordinary row added later is not exempt.
CENSUS_MIN, CENSUS_MIN_SHARE = 10000, 1000
LOWER_EDGE = {(entry, tuple(args[:5]) + (0,) if entry in ("conv", "film") else tuple(args)) for entry, args, _, _, _ in TINY_CASES}


def lower_edge(r: Row) -> bool:
    return (r.entry, tuple(r.args[:5]) + (0,) if r.entry in ("conv", "film") else r.args) in LOWER_EDGE


def row_id(r: Row) -> str:
    return "-".join([r.entry, "x".join(str(v) for v in r.args), r.dt] + (["silu"] if r.silu else []) + [f"{k[3:]}={v}" for k, v in r.env.items()])


# ---- integer tensors --------------------------------------------------------------------------------------------------------------
def ints(shape, a: int, seed: int, scale: float = 1.0) -> torch.Tensor:
    """Seeded integers of [-a, a] (times a power-of-two `scale`) as float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-a, a + 1, tuple(shape), generator=g).float() * scale


def choice(shape, values, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), tuple(shape), generator=g)]


def taps_inside(H: int, W: int, k: int = 3) -> int:
    """The most taps of a k x k window (pad 1 for k = 3) that fall inside an H x W image: 9 from 3 x 3 on, 1 on a 1 x 1 image, where
    only the centre tap's products are real and the output's spread is a third of what 9 taps give."""
    return min(k, H) * min(k, W)


def conv_ax(nterms: int, dt: str, big: bool, full: int = 0) -> int:
    """Activation amplitude of a convolution over `nterms` products (taps inside the image x channels) with weights of [-AW, AW].  ax = 15
    where bf16 / f32 suffice (outputs of a few hundred: bf16 rounds integers from 256 on); where an image is too small for all `full`
    products of the window (`nterms` < `full`) the amplitude grows by sqrt(full / nterms), so that the outputs keep that spread.  `big`
    (f16, SiLU): the output's standard deviation, sqrt(nterms) ax AW / 3 for uniform integers, reaches SIGMA."""
    if not big:
        return min(INT_MAX[dt], math.ceil(15 * math.sqrt(max(full, nterms) / nterms)))
    return min(INT_MAX[dt], max(15, math.ceil(3.0 * SIGMA / (AW * math.sqrt(nterms)))))


def gate_aw(c: int, mean_abs_x: float, mean_abs_z: float) -> int:
    """Gate weights are GATE_SCALE * [-aw, aw]: the largest aw <= AW whose expected sum of absolute products over [x ; z] -- c terms each,
    mean |w| = GATE_SCALE aw / 2 -- stays below half of 2^24: the largest sum over the pixels of a row lies well above the mean (the
    CPU test checks the true maximum)."""
    return max(1, min(AW, int(0.5 * EXACT_SUM / (c * GATE_SCALE * 0.5 * (mean_abs_x + mean_abs_z)))))


# ---- one rounding, on the bit pattern -----------------------------------------------------------------------------------------------
FORMAT = {"f32": (23, 127, 8), "bf16": (7, 127, 8), "f16": (10, 15, 5)}  # mantissa bits, exponent bias, exponent bits


def _round_parts(y64: torch.Tensor, dt: str):
    """(bit pattern of y rounded to nearest even in `dt`, inexact, exact tie, rounded away from zero) as numpy arrays.  Integer
    arithmetic on the float64 bit pattern: 53-bit significand, shifted right by what the target cannot hold (more below its smallest
    normal exponent), remainder against half."""
    M, bias, ebits = FORMAT[dt]
    emin = 1 - bias
    a = np.ascontiguousarray(y64.detach().cpu().to(torch.float64).numpy())
    assert np.isfinite(a).all()
    bits = a.view(np.int64)
    sign = (bits >> 63) & 1
    e = (bits >> 52) & 0x7FF
    assert not ((e == 0) & ((bits & ((1 << 52) - 1)) != 0)).any(), "float64 subnormals are not handled"
    sig = (bits & ((1 << 52) - 1)) | (np.int64(1) << 52)
    E = e - 1023
    Et = np.maximum(E, emin)  # exponent of the target's leading bit position
    shift = np.minimum(52 - M + (Et - E), 62)  # >= 54: everything is remainder, below half
    q = sig >> shift
    rem = sig & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    zero = e == 0
    tie = (rem == half) & ~zero
    up = ((rem > half) | (tie & ((q & 1) == 1))) & ~zero
    inexact = (rem != 0) & ~zero
    q = q + up
    # normal: field = Et + bias, mantissa q - 2^M (q = 2^(M+1) carries into the field by itself); subnormal: field 0, mantissa q
    normal = E >= emin
    out = np.where(normal, ((Et + bias) << M) + (q - (1 << M)), q)
    inf = ((1 << ebits) - 1) << M
    out = np.where(out >= inf, inf, out)
    out = np.where(zero, 0, out)
    out = out | (sign << (M + ebits))
    return out, inexact, tie, up


def round_once(y64: torch.Tensor, dt: str) -> torch.Tensor:
    """float64 -> `dt`, rounded to nearest even ONCE."""
    out, _, _, _ = _round_parts(y64, dt)
    if dt == "f32":
        return torch.from_numpy(out.astype(np.uint32).view(np.int32)).view(torch.float32).reshape(y64.shape)
    return torch.from_numpy(out.astype(np.uint16).view(np.int16)).view(DTYPES[dt]).reshape(y64.shape)


def census(y64: torch.Tensor, dt: str):
    """Shares of elements that (need rounding, are exact ties, round differently under truncation than under nearest-even)."""
    _, inexact, tie, up = _round_parts(y64, dt)
    n = max(1, inexact.size)
    return inexact.sum() / n, tie.sum() / n, up.sum() / n


def bits_of(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
class Exact:
    """One row's data: `inputs` (float32 CPU tensors by argument name, integer-valued or as the entry states), `alpha`, `C` (real
    output channels; None: a dense image), `y64` (what is rounded), `want` (storage type), `keep` (None: every element is compared for
    equality; else the mask of those that are), `soft64` (the float64 formula, for the excluded elements), `sums` (largest sum of
    absolute products per accumulated quantity), `branches` (shares of the two saturated branches)."""

    def __init__(self):
        self.alpha, self.keep, self.soft64, self.sums, self.branches = 0.0, None, None, {}, None

    @property
    def excluded(self) -> float:
        return 0.0 if self.keep is None else 1.0 - self.keep.double().mean().item()

    def compared(self) -> torch.Tensor:
        return self.y64 if self.keep is None else self.y64[self.keep]


def _saturate(ex: Exact, t64, one64, zero64, soft64):
    """t: the transcendental's argument.  one64 / zero64: the result where the sigmoid is exactly 1 / exactly 0."""
    hi, lo = t64 >= SAT_HI, t64 <= SAT_LO
    ex.keep = hi | lo
    ex.y64 = torch.where(hi, one64, zero64)
    ex.soft64 = soft64
    ex.branches = (hi.double().mean().item(), lo.double().mean().item())


def finish(ex: Exact, entry, args, dt, silu=0, gate=None) -> Exact:
    """The shared end of every builder, on the drawn ex.inputs: C, the float64 reference, the sums of absolute products, the saturation
    of a transcendental and the expected storage-type tensor, all from the entry's statement in tests/op_ref.py.  gate(ex, mix): the
    gate that classifies the elements of a mix where that is not the mix's own; it then states the mix's sums itself."""
    t = {k: v.double() for k, v in ex.inputs.items()}
    op_ref.check_shapes(entry, args, t)
    ex.C, shape = op_ref.output(entry, args)
    ex.sums.update(op_ref.abs_sums(entry, t))
    if entry in op_ref.MIXES:
        m = op_ref.Mix(entry, t, lambda z: round_once(z, dt).double())
        if entry == "conv_mix":
            ex.z64_unrounded = m.z_raw
        ex.z64 = m.z
        if gate is None:
            ex.sums.update(m.abs_sums())
        # alpha = 0: sigmoid(alpha) = 1/2 and the host's 1 + e^-alpha = 2 are exact
        _saturate(ex, m.gate if gate is None else gate(ex, m), (m.x + m.z) / 2, m.x, m.x + 0.5 * torch.sigmoid(m.gate) * (m.z - m.x))
    else:
        y = op_ref.reference(entry, args, t, silu=False)
        if silu:  # t >= SAT_HI: t * 1; t <= SAT_LO: t * 0
            _saturate(ex, y, y, torch.zeros_like(y), F.silu(y))
        else:
            ex.y64 = y
    assert tuple(ex.y64.shape) == shape, (entry, args)
    ex.want = round_once(ex.y64, dt)
    return ex


def _build(entry, args, dt, silu) -> Exact:
    """The recipe of the exact rows: which numbers each of the entry's inputs (op_ref.shapes) holds."""
    ex = Exact()
    a, s = fields(entry, args), op_ref.shapes(entry, args)
    big = dt == "f16" or bool(silu)
    if entry in ("conv", "film", "d2s", "crush"):
        k = s["w"][-1]
        nterms = taps_inside(a.H, a.W, k) * a.cin * (4 if entry == "film" else 1)  # film: |gamma| <= 2 doubles the spread, as four times the terms would
        full = k * k * a.cin * (4 if entry == "film" else 1)
        ex.inputs = {"in0": ints(s["in0"], conv_ax(nterms, dt, big, full), 101), "w": ints(s["w"], AW, 102)}
        if entry == "film":
            ex.inputs.update(gamma=choice(s["gamma"], [-1.0, 0.5, 1.0, 2.0], 103), beta=ints(s["beta"], 8, 104))
    elif entry == "stem":
        ex.inputs = {"x": ints(s["x"], INT_MAX[dt], 105).abs(), "w": choice(s["w"], [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], 106), "b": ints(s["b"], 8, 107)}
    elif entry == "final":
        ex.inputs = {"feat": ints(s["feat"], conv_ax(taps_inside(a.H, a.W) * a.cin, dt, big, 9 * a.cin), 108),
                     "img": torch.zeros(s["img"]),  # the bicubic term is exactly zero
                     "w": ints(s["w"], AW, 109)}
    elif entry == "mix":
        ax = INT_MAX[dt]  # x: every integer the type holds
        # z: multiples of 4, so that (x + z) / 2 = x / 2 + 2 zi needs rounding (exact, tie or neither by x mod 4) in both 16-bit types
        az = 255 if dt == "bf16" else 511
        ex.inputs = {"in0": ints(s["in0"], ax, 110), "in1": ints(s["in1"], az, 111, 4.0),
                     "w": ints(s["w"], gate_aw(a.C, ax / 2.0, 2.0 * az), 115, float(GATE_SCALE))}
    elif entry == "conv_mix":
        ax = INT_MAX[dt]
        nterms = taps_inside(a.H, a.W) * a.cin
        ah = conv_ax(nterms, dt, big, 9 * a.cin)
        mean_z = 0.8 * math.sqrt(nterms) * ah * AW / 3.0  # E|z| of a normal variable
        ex.inputs = {"hid": ints(s["hid"], ah, 112), "x": ints(s["x"], ax, 113), "w2": ints(s["w2"], AW, 114),
                     "wmix": ints(s["wmix"], gate_aw(a.cout, ax / 2.0, mean_z), 115, float(GATE_SCALE))}
    else:
        raise ValueError(entry)
    return finish(ex, entry, args, dt, silu)


@functools.lru_cache(maxsize=None)
def _cached(entry, args, dt, silu):
    return _build(entry, args, dt, silu)


def exact(r: Row) -> Exact:
    """The row's data, built once (rows that differ in their knobs share it) and never changed."""
    return _cached(r.entry, r.args, r.dt, r.silu)


ROWS = _rows()

# Persistent families once more under MZ_PERSIST_WGS = 8 and 16 (on these shapes a workgroup then walks several tiles, in two different
# splits).  Rows whose tiles do not outnumber the workgroups fall back to a per-tile family under that knob and are left out:
# tests/test_exact_cpu.py checks that every walk listed here keeps its row's family.
WALK_WGS = (8, 16)
NOT_PERSISTENT_AT_16 = {(1, 20, 130, 112, 96, 0)}  # conv3p: nine 8 x 64 tiles do not outnumber 16 workgroups
# nor do the one-tile images of the lower edge: of their conv3p rows only 16 images of Cout = 288 (nine N tiles each) keep the family
NOT_PERSISTENT_AT_16 |= {(3, 1, 1, 16, 288, 0), (3, 1, 9, 16, 288, 0), (3, 9, 1, 16, 288, 0), (3, 2, 3, 16, 288, 0), (16, 1, 1, 112, 96, 0)}
WALKS = [(r, n) for r in ROWS for n in WALK_WGS
         if r.kernel in PERSISTENT and "MZ_NO_PERSIST" not in r.env and r.env.get("MZ_PERSIST_WGS") != str(n)
         and not (n == 16 and r.kernel == "conv3p" and r.args in NOT_PERSISTENT_AT_16)]


def walk_id(w) -> str:
    return f"{row_id(w[0])}-walk{w[1]}"
