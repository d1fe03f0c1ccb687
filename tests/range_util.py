"""Number-range test data (tests/test_range_cpu.py, tests/test_range_gpu.py).  Needs no GPU.

tests/exact_util.py fixes every family's arithmetic bit for bit, but in one band of the number line: integers of a few thousand at the
most, every rounding in the normal range.  This module puts the same rows (the rows of ordinary size of exact_util.ROWS: every family x
dtype x knob set pinned there) at the ends of the storage type, and sweeps the argument range of the transcendentals:

  SMALL   inputs are integers times a power of two that puts them at the BOTTOM of the type.  Every product and partial sum is still an
          exact f32 value (the sum of absolute products stays below 2^24 units of the product grid), so the output must equal the
          float64 result rounded ONCE, into the subnormal range where it lies there.  Variants:
            f16 "xsub"   activations n 2^-24, |n| <= 1023 (all subnormal), weights m 2^-6
            f16 "wsub"   weights m 2^-24 (all subnormal), activations n 2^-8, |n| <= 2047
            bf16 "sub"   activations n 2^-133, |n| <= 127 (all subnormal), weights m 2^-4: the products are f32 SUBNORMALS
            f32 "sub"    activations n 2^-149, integer weights.  Every output is an f32 subnormal and needs no rounding: a product on a
                         finer grid would be no f32 value, so this variant fixes PASS-THROUGH only (no flush anywhere on the way),
                         not a rounding.  Where an operator halves (the stem's weights, the blend's 1/2) the grid is 2^-148.
  LARGE   f16 only, the entries that end in a plain store (conv, d2s, crush, film, stem, final): integer data whose outputs straddle
          65504.  f32 accumulation stays exact, the expectation is round_once: +-inf from the tie 65520 upward.  Left out: mix and
          conv_mix (an infinite z makes the reference NaN), and bf16 / f32, whose overflow band lies within half a bf16 ulp of FLT_MAX
          and cannot be reached without overflowing partial sums.
  WINDOW  SiLU and the gate on EVERY finite value of the storage type inside (SAT_LO, SAT_HI) = (-100, 32), both zeros and all
          subnormals included, through one-hot weights (the convolution is the identity), against float64 with a derived bound.

What the small variants leave out, and why: the mix entry and the stem have no "wsub" variant (the mix's only weights are the gate's,
which saturate or they are nothing; the stem's weights travel as f32), and the SiLU rows have none either (activations of 8 times
subnormal weights cannot reach an argument of 32).

The gate of a mix cannot saturate on subnormal data alone: DRIVERS channels of x carry exact_util's integers and their gate columns
its x16 weights; every other channel of x and all of z (hid) are at the subnormal scale, and the gate's other columns are m 2^-10.
z is ZERO in the driver channels (the conv_mix rows: zero rows of w2): x + z of an integer of 2^11 and a value of 2^-24 is no f32 value,
so the blend's z - x would round a second time there.  The expectation classifies every element by the driver-only gate;
tests/test_range_cpu.py proves that the other channels move no gate by more than GATE_SHIFT = 2^-10, far inside the margin of both
thresholds (e^-(32 - 2^-10) is still below 2^-46, e^100 overflows f32 by eleven decades).  The SiLU rows (conv3r's ragged variant) are
saturated without drivers: non-negative subnormal activations, weights of one sign per output channel at the top of the type's range
(m 2^13, m 2^125), so that t keeps a magnitude of a few hundred while every x is subnormal; their outputs are t or 0, not subnormal."""

from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import op_ref
from exact_util import AW, GATE_SCALE, INT_MAX, ROWS, SAT_HI, SAT_LO, Exact, Row, _round_parts, choice, finish, ints, lower_edge, row_id, taps_inside
from gpu_util import DTYPES
from op_cases import ALL, CASES, LOW, TINY_CASES, fields
from op_ref import MIXES, abs_sum

MIN_NORMAL = {"f32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -14}
MANTISSA = {"f32": 23, "bf16": 7, "f16": 10}
VARIANTS = {"f16": ("xsub", "wsub"), "bf16": ("sub",), "f32": ("sub",)}
# (dtype, variant) -> (activation scale, activation amplitude, weight scale)
SCALE = {("f16", "xsub"): (2.0 ** -24, 1023, 2.0 ** -6), ("f16", "wsub"): (2.0 ** -8, 2047, 2.0 ** -24),
         ("bf16", "sub"): (2.0 ** -133, 127, 2.0 ** -4), ("f32", "sub"): (2.0 ** -149, 127, 1.0)}
HALVING = ("stem", "mix", "conv_mix")  # f32: these entries halve a value, their activations are EVEN multiples of 2^-149
SILU_WS = {"f16": 2.0 ** 13, "bf16": 2.0 ** 125}  # the SiLU rows' weight scale: |w| <= 7 * that is still a value of the type
DRIVERS = 4
GATE_REST = 2.0 ** -10   # scale of the gate's columns that are no driver's
GATE_SHIFT = 2.0 ** -10  # the most they may move any gate
# floors of the share of an input tensor that is subnormal (non-zero, below the smallest normal): integers of [-a, a] are zero with
# probability 1 / (2 a + 1): at most 1/255 of the activations (the smallest tensor, 192 pixels, may hold three), 1/15 of the weights
FLOOR_X, FLOOR_W = 0.98, 0.90
# census floors among compared outputs (tests/test_range_cpu.py)
MIN_SUB_SHARE, MIN_SUB_INEXACT, MIN_SUB_TIES = 0.10, 100, 30

Small = namedtuple("Small", "row variant")
STORE_ENTRIES = ("conv", "d2s", "crush", "film", "stem", "final")


def _small_rows():
    out = []
    for r in ROWS:
        if lower_edge(r):
            continue
        for v in VARIANTS[r.dt]:
            if v == "wsub" and (r.entry in ("mix", "stem") or r.silu):
                continue
            out.append(Small(r, v))
    return out


def small_id(s: Small) -> str:
    return f"{row_id(s.row)}-{s.variant}"


def is_sub(t: torch.Tensor, dt: str) -> torch.Tensor:
    """Non-zero and below the smallest normal of `dt`."""
    return (t != 0) & (t.abs().double() < MIN_NORMAL[dt])


def drivers(c: int):
    return [0, c // 3, (2 * c) // 3, c - 1][:DRIVERS]


# ---- SMALL ---------------------------------------------------------------------------------------------------------------------------
def _gate_weights(c, seed):
    """The driver construction (module docstring): x16 integers in the drivers' columns, m 2^-10 in every other."""
    drv = drivers(c)
    wmix = ints((c, 2 * c, 1, 1), AW, seed, GATE_REST)
    wmix[:, drv] = ints((c, len(drv), 1, 1), AW, seed + 1, float(GATE_SCALE))
    return wmix


def _drivers_gate(ex: Exact, m, sx):
    """The driver-only gate, which classifies, and the bound of what the rest moves; the blend's sum over the channels that are no
    drivers', in units of the activations' scale `sx` (x and the rounded z are multiples of it)."""
    c = m.x.shape[1]
    drv = drivers(c)
    only = torch.zeros_like(m.xz)
    only[:, drv] = m.xz[:, drv]
    ex.sums["gate"] = abs_sum(only, m.w)
    ex.gate_shift = abs_sum(m.xz - only, m.w)
    ex.rest = torch.ones(c, dtype=torch.bool)
    ex.rest[drv] = False
    ex.sums["blend"] = (m.x.abs() + m.z.abs())[:, ex.rest].max().item() / sx
    return F.conv2d(only, m.w)


def _build_small(entry, args, dt, silu, variant) -> Exact:
    ex = Exact()
    s = op_ref.shapes(entry, args)
    xs, ax, ws = SCALE[(dt, variant)]
    if dt == "f32" and entry in HALVING:
        xs *= 2.0
    ex.grid = xs * ws       # the product grid of the 3x3 / 2x2 convolution
    ex.subnormal = {}       # input name -> (share of it that is subnormal, the floor its variant states)
    xfloor = FLOOR_X if variant != "wsub" else None
    wfloor = FLOOR_W if variant == "wsub" else None

    def note(name, t, floor, channels=None):
        if floor is not None:
            t = t if channels is None else t[:, channels]
            ex.subnormal[name] = (is_sub(t, dt).double().mean().item(), floor)

    if entry in ("conv", "film", "d2s", "crush"):
        x, w = ints(s["in0"], ax, 201, xs), ints(s["w"], AW, 202, ws)
        if silu:  # saturated without drivers (module docstring)
            assert entry == "conv" and variant != "wsub"
            sign = torch.where(torch.arange(s["w"][0]) % 2 == 0, 1.0, -1.0)[:, None, None, None]
            x, w = x.abs(), ints(s["w"], AW, 202, SILU_WS[dt]).abs() * sign
            ex.grid = xs * SILU_WS[dt]
        ex.inputs = {"in0": x, "w": w}
        note("in0", x, xfloor)
        note("w", w, wfloor)
        if entry == "film":  # gamma as exact_util's, beta on the product grid
            ex.inputs.update(gamma=choice(s["gamma"], [-1.0, 0.5, 1.0, 2.0], 203), beta=ints(s["beta"], 8, 204, ex.grid))
    elif entry == "stem":
        ex.grid = xs / 2
        ex.inputs = {"x": ints(s["x"], ax, 205, xs).abs(), "w": choice(s["w"], [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], 206), "b": ints(s["b"], 8, 207, xs)}
        note("x", ex.inputs["x"], xfloor)
    elif entry == "final":
        ex.inputs = {"feat": ints(s["feat"], ax, 208, xs),
                     "img": torch.zeros(s["img"]),  # the bicubic term is exactly zero
                     "w": ints(s["w"], AW, 209, ws)}
        note("feat", ex.inputs["feat"], xfloor)
        note("w", ex.inputs["w"], wfloor)
    elif entry in MIXES:
        xname = "in0" if entry == "mix" else "x"
        B, c, H, W = s[xname]
        drv = drivers(c)
        rest = [i for i in range(c) if i not in drv]
        # x at the bottom of the type (the "wsub" variant's, too: its activations of 2^-8 belong to hid), integers in the driver channels
        sx, amp = (2.0 ** -24, 1023) if variant == "wsub" else (xs, ax)
        x = ints(s[xname], amp, 210, sx)
        x[:, drv] = ints((B, len(drv), H, W), INT_MAX[dt], 211)
        if entry == "mix":
            z = ints(s["in1"], ax, 212, xs)
            z[:, drv] = 0.0
            ex.inputs = {"in0": x, "in1": z, "w": _gate_weights(c, 215)}
            note("in0", x, FLOOR_X, rest)
            note("in1", z, FLOOR_X, rest)
        else:
            hid, w2 = ints(s["hid"], ax, 213, xs), ints(s["w2"], AW, 214, ws)
            w2[drv] = 0.0
            ex.inputs = {"hid": hid, "x": x, "w2": w2, "wmix": _gate_weights(c, 215)}
            note("x", x, FLOOR_X, rest)
            note("hid", hid, xfloor)
            note("w2", w2[rest], wfloor)
    else:
        raise ValueError(entry)
    finish(ex, entry, args, dt, silu, gate=functools.partial(_drivers_gate, sx=sx) if entry in MIXES else None)
    for name, unit in (("conv", ex.grid), ("film", ex.grid / 2), ("stem", ex.grid)):  # in units of the quantity's grid
        if name in ex.sums:
            ex.sums[name] /= unit
    return ex


@functools.lru_cache(maxsize=None)
def _cached_small(entry, args, dt, silu, variant):
    return _build_small(entry, args, dt, silu, variant)


def small(s: Small) -> Exact:
    """The row's data at the bottom of its type, built once and never changed."""
    r = s.row
    return _cached_small(r.entry, r.args, r.dt, r.silu, s.variant)


def sub_census(y64: torch.Tensor, dt: str):
    """Among the values y (float64, before the rounding): (share that is subnormal in `dt` after it or on the way to it, count of those
    that need rounding, count of exact ties among them, count that truncation would round differently)."""
    _, inexact, tie, up = _round_parts(y64, dt)
    a = y64.detach().abs().numpy()
    sub = (a != 0) & (a < MIN_NORMAL[dt])
    return sub.sum() / max(1, sub.size), int((sub & inexact).sum()), int((sub & tie).sum()), int((sub & up).sum())


SMALL = _small_rows()
# Rows too small for the census' counts (exact_util's LOWER_EDGE rule; "wsub" rounds eight bits away, one output in 256 is a tie): they
# are held to every other condition and to at least one subnormal output that tells truncation from nearest-even, and their family's
# counts are pinned by a row of ordinary size of the same entry, family, type and variant, which tests/test_range_cpu.py checks exists.
# Named one by one: (entry, arguments, variant; None: every variant).
SMALL_LEAN = {("conv", (1, 5, 9, 160, 16, 0), None), ("conv", (3, 5, 9, 160, 16, 0), None), ("crush", (1, 21, 19, 24, 40), "wsub"),
              ("final", (2, 9, 11, 16, 2), "wsub"), ("final", (3, 9, 11, 16, 2), "wsub"), ("final", (1, 16, 24, 32, 8), "wsub")}


def lean(s: Small) -> bool:
    return (s.row.entry, s.row.args, s.variant) in SMALL_LEAN or (s.row.entry, s.row.args, None) in SMALL_LEAN


# ---- LARGE ---------------------------------------------------------------------------------------------------------------------------
F16_MAX, F16_TIE = 65504.0, 65520.0
LARGE_SIGMA = 50000.0  # standard deviation of the outputs: a normal variable passes 65520 with probability 0.19
PLANT = ((2047.0, 16.0), (2047.0, 15.0), (-2047.0, -16.0))  # 32 a + b = 65520 (the tie: +inf), 65519 (65504), -65520 (-inf)
LARGE = [r for r in ROWS if not lower_edge(r) and r.dt == "f16" and r.entry in STORE_ENTRIES and not r.silu]


def large_ax(nterms: int) -> int:
    """Uniform integers of [-ax, ax] (deviation ax / sqrt 3) times weights of [-AW, AW] (deviation 4.3), `nterms` products."""
    return min(INT_MAX["f16"], math.ceil(LARGE_SIGMA * math.sqrt(3.0) / (4.3 * math.sqrt(nterms))))


def _plant(x, w, tap, step):
    """Output channel 0 becomes 32 x[0] + x[1] at `tap`; three pixels of image 0's first row carry PLANT (`step` apart: 2 for the 2x2
    gather, whose windows do not overlap)."""
    assert x.shape[3] > 2 * step
    w[0] = 0.0
    w[(0, 0) + tap], w[(0, 1) + tap] = 32.0, 1.0
    for i, (p, q) in enumerate(PLANT):
        x[0, 0, 0, i * step], x[0, 1, 0, i * step] = p, q


def _build_large(entry, args) -> Exact:
    ex = Exact()
    a, s = fields(entry, args), op_ref.shapes(entry, args)
    if entry in ("conv", "film", "d2s", "crush"):
        k = s["w"][-1]
        nterms = taps_inside(a.H, a.W, k) * a.cin * (1.5 if entry == "film" else 1)  # film: gamma of {-1, 1/2, 1, 2} has a mean square of 1.56
        x, w = ints(s["in0"], large_ax(nterms), 301), ints(s["w"], AW, 302)
        _plant(x, w, (0, 0) if k == 2 else (1, 1), 2 if k == 2 else 1)
        ex.inputs = {"in0": x, "w": w}
        if entry == "film":
            gamma, beta = choice(s["gamma"], [-1.0, 0.5, 1.0, 2.0], 303), ints(s["beta"], 8, 304)
            gamma[0, 0], beta[0, 0] = 1.0, 0.0
            ex.inputs.update(gamma=gamma, beta=beta)
    elif entry == "stem":  # the weights travel as f32: exact_util's times 16, or three pixels of 2047 could not reach 65504
        x = ints(s["x"], INT_MAX["f16"], 305).abs()
        w, b = choice(s["w"], [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], 306) * 16.0, ints(s["b"], 8, 307)
        w[0, :, 0, 0], w[1, :, 0, 0] = torch.tensor([32.0, 1.0, 0.0]), torch.tensor([-32.0, -1.0, 0.0])
        b[0] = b[1] = 0.0
        for i, (p, q) in enumerate(PLANT[:2]):
            x[0, 0, 0, i], x[0, 1, 0, i] = p, q
        ex.inputs = {"x": x, "w": w, "b": b}
    elif entry == "final":
        feat, w = ints(s["feat"], large_ax(taps_inside(a.H, a.W) * a.cin), 308), ints(s["w"], AW, 309)
        _plant(feat, w, (1, 1), 1)
        ex.inputs = {"feat": feat, "img": torch.zeros(s["img"]), "w": w}
    else:
        raise ValueError(entry)
    return finish(ex, entry, args, "f16")


@functools.lru_cache(maxsize=None)
def _cached_large(entry, args):
    return _build_large(entry, args)


def large(r: Row) -> Exact:
    return _cached_large(r.entry, r.args)


# ---- WINDOW --------------------------------------------------------------------------------------------------------------------------
def window_values(dt: str) -> torch.Tensor:
    """Every finite value t of `dt` with SAT_LO < t < SAT_HI as float32, both zeros and all subnormals included; f32: the union of the
    two 16-bit sets (as distinct BIT PATTERNS: both zeros stay)."""
    if dt == "f32":
        both = torch.cat([window_values("bf16"), window_values("f16")])
        return torch.from_numpy(np.unique(both.numpy().view(np.int32))).view(torch.float32)
    v = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(DTYPES[dt]).float()
    return v[torch.isfinite(v) & (v > SAT_LO) & (v < SAT_HI)]


def _random_f32(n: int, seed: int) -> torch.Tensor:
    """Seeded random f32 BIT PATTERNS inside the window."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(0)
    while out.numel() < n:
        v = torch.randint(-2 ** 31, 2 ** 31, (2 * n + 64,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
        out = torch.cat([out, v[torch.isfinite(v) & (v > SAT_LO) & (v < SAT_HI)]])
    return out[:n]


def _fill(n: int, dt: str, seed: int) -> torch.Tensor:
    """n >= |window| values: every window value once, in a seeded order, then repeats (f32: random bit patterns)."""
    vals = window_values(dt)
    assert n >= vals.numel(), (n, vals.numel())
    g = torch.Generator().manual_seed(seed)
    more = n - vals.numel()
    extra = _random_f32(more, seed + 1) if dt == "f32" else vals[torch.randint(0, vals.numel(), (more,), generator=g)]
    all_ = torch.cat([vals, extra])
    return all_[torch.randperm(n, generator=g)]


def window_B(dt: str, per_image: int, B: int) -> int:
    """The row's B raised until the channels that are read hold the window (f32: and a fifth as many random patterns)."""
    need = window_values(dt).numel() * (1.2 if dt == "f32" else 1.0)
    return max(B, math.ceil(need / per_image))


def ulp64(v: torch.Tensor, dt: str) -> torch.Tensor:
    """Spacing of `dt` at |v| (float64), the subnormal spacing below the smallest normal."""
    _, e = torch.frexp(v.abs().double())
    emin = round(math.log2(MIN_NORMAL[dt]))
    e = torch.where(v == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - MANTISSA[dt])


# |got - want| <= 0.5 ulp_dt(|want|) + REL * scale + FLUSH.  REL is twice the chain's derived worst relative error: rounding the product
# t * log2(e) at |t| up to 100 moves the exponential by 100 * 2^-24 = 2^-17.3, the four 1-ulp / half-ulp steps (v_exp_f32, the add,
# v_rcp_f32, the last product or fma) add 3 * 2^-24.  FLUSH admits a result flushed where an intermediate is an f32 subnormal (t near
# -88).  No absolute floor.  scale: |want| for SiLU, |x| + |z - x| for the blend.
REL, FLUSH = 2.0 ** -16, 2.0 ** -126
# The contract's one exception (include/mewzoom_hip.h, "number range"), a property of the transcendental unit, not of this code: v_rcp_f32
# returns ZERO where its result would be an f32 subnormal.  Measured on gfx950 by this sweep: SiLU(t) came out as -0 for every t of
# (-88.72, -87.34) (sigmoid(t) < 2^-126; want about -88 * 2^-126, 59 to 84 times the bound above, whose FLUSH term is additive and
# forgets the factor t), in every SiLU family alike, builtin and inline-asm copies; below -88.72 the exponential overflows and the
# result is zero anyway.  So where the reciprocal's true value (sigmoid(t) in SiLU, sigmoid(t) / 2 in the gate at alpha = 0) lies below
# RCP_MIN -- times 1 + REL: the chain's own error decides on which side of the threshold it lands -- the result may ALSO be the one the
# float64 formula gives with that factor taken as zero: 0 for SiLU, x for the blend.  Nowhere else, and never taken from a kernel.
RCP_MIN = 2.0 ** -126


def window_ratio(got: torch.Tensor, want64: torch.Tensor, scale64: torch.Tensor, dt: str, may_flush=None, flushed64=None) -> torch.Tensor:
    """|got - want| / bound, element-wise (float64); <= 1 passes.  may_flush / flushed64: where, and to what, the reciprocal's flush may
    take the result instead (the smaller of the two ratios counts there)."""
    g = got.double()
    ratio = (g - want64).abs() / (0.5 * ulp64(want64, dt) + REL * scale64 + FLUSH)
    if may_flush is not None:
        alt = (g - flushed64).abs() / (0.5 * ulp64(flushed64, dt) + REL * scale64 + FLUSH)
        ratio = torch.where(may_flush, torch.minimum(ratio, alt), ratio)
    return ratio


# a window row: one call of an entry on the window's values (kernel: the family the host chooses for it, checked without a GPU by
# tests/test_range_cpu.py)
Win = namedtuple("Win", "entry args env dt kernel")


def win_id(w: Win) -> str:
    return "-".join([w.entry, "x".join(str(v) for v in w.args), w.dt] + [f"{k[3:]}={v}" for k, v in w.env.items()])


_TINY = {(e, a) for e, a, _, _, _ in TINY_CASES}


def _ordinary_cases():
    """CASES of ordinary size, without the B = 3 twins op_cases.add() appends to every row."""
    seen, out = set(), []
    for entry, args, env, dt, kernel in CASES:
        if (entry, args) in _TINY:
            continue
        key = (entry, args[1:], tuple(env.items()), dt)
        if key in seen:
            continue
        seen.add(key)
        out.append((entry, args, env, dt, kernel))
    return out


# SiLU rows: a shape of op_cases per family that applies SiLU, run with silu = 1 (tests/test_range_cpu.py checks without a GPU that the
# name is the host's choice there, and that every family of op_cases' conv rows has one).  Rows on the same shape and type whose knobs
# choose different families are TWINS: those families promise identical bits (silu2 of conv3s against silu_pair_to and the scalar
# form of conv3r's helper role, mz_relay.h / mz_conv3r.h; silu_pair_to of conv3t), and their outputs are compared with each other, too.
SILU_SHAPES = [("conv", (1, 24, 48, 96, 80), {}, "conv3r", LOW), ("conv", (1, 24, 48, 96, 80), {"MZ_NO_R": "1"}, "conv3s", LOW),
               ("conv", (2, 13, 37, 128, 96), {}, "conv3r_8x40", LOW), ("conv", (2, 13, 37, 128, 96), {"MZ_NO_R": "1"}, "conv3s", LOW),
               ("conv", (2, 13, 37, 48, 192), {}, "conv3r_ragged", LOW),
               ("conv", (2, 13, 37, 96, 48), {}, "conv3t", LOW), ("conv", (2, 13, 37, 96, 48), {"MZ_NO_T": "1"}, "conv3s", LOW),
               ("conv", (3, 33, 65, 16, 288), {"MZ_PERSIST_WGS": "8"}, "conv3p", ALL),
               ("conv", (2, 13, 37, 16, 48), {"MZ_NO_PERSIST": "1"}, "conv3w", ALL),
               ("conv", (1, 9, 33, 24, 40), {"MZ_NO_WIDE": "1"}, "conv_kernel", ALL),
               ("film", (3, 9, 33, 64, 40), {}, "conv3s", LOW)]


def _silu_rows():
    out = []
    for entry, (B, H, W, cin, cout), env, kernel, dts in SILU_SHAPES:
        for dt in dts:
            out.append(Win(entry, (window_B(dt, min(cin, cout) * H * W, B), H, W, cin, cout, 1), env, dt, kernel))
    return out


def _gate_rows():
    """Every mix and conv_mix row of ordinary size of op_cases, B raised until x holds the window."""
    out = []
    for entry, args, env, dt, kernel in _ordinary_cases():
        if entry not in ("mix", "conv_mix"):
            continue
        f = fields(entry, args)
        B = window_B(dt, op_ref.output(entry, args)[0] * f.H * f.W, f.B)
        out.append(Win(entry, (B,) + tuple(args[1:]), env, dt, kernel))
    return out


SILU_WINDOW = _silu_rows()
GATE_WINDOW = _gate_rows()


# SiLU rows on one input (same entry, arguments and type) whose knobs choose different families
SILU_TWINS = [(p, q) for i, p in enumerate(SILU_WINDOW) for q in SILU_WINDOW[i + 1:]
              if (p.entry, p.args, p.dt) == (q.entry, q.args, q.dt) and p.kernel != q.kernel]


class Window:
    """inputs (float32 CPU tensors by argument name), x64 (the swept argument per OUTPUT element), z64 (gate rows), want64, scale64,
    may_flush and flushed64 (window_ratio)."""


@functools.lru_cache(maxsize=None)
def _cached_window(entry, args, dt):
    wd = Window()
    d = lambda t: t.double()
    a = fields(entry, args)
    B, H, W = a.B, a.H, a.W
    wd.C = c = op_ref.output(entry, args)[0]
    if entry in ("conv", "film"):
        cin, cout = a.cin, c
        nread = min(cin, cout)
        x = torch.empty(B, cin, H, W)
        x[:, :nread] = _fill(B * nread * H * W, dt, 401).reshape(B, nread, H, W)
        x[:, nread:] = 1.0  # never read: their weights are zero
        w = torch.zeros(cout, cin, 3, 3)
        src = torch.arange(cout) % cin
        w[torch.arange(cout), src, 1, 1] = 1.0
        wd.inputs = {"in0": x, "w": w}
        if entry == "film":
            wd.inputs.update(gamma=torch.ones(B, cout), beta=torch.zeros(B, cout))
        wd.x64 = d(x)[:, src]
        wd.want64 = wd.x64 * torch.sigmoid(wd.x64)
        wd.scale64 = wd.want64.abs()
        wd.may_flush, wd.flushed64 = torch.sigmoid(wd.x64) < RCP_MIN * (1 + REL), 0.0 * wd.x64
        wd.read = x[:, :nread]
    else:
        n = B * c * H * W
        x = _fill(n, dt, 411).reshape(B, c, H, W)
        g = torch.Generator().manual_seed(412)
        zc = x.flatten()[torch.randperm(n, generator=g)].reshape(B, c, H, W)  # a fixed permutation of the same values
        wmix = torch.zeros(c, 2 * c, 1, 1)
        wmix[torch.arange(c), torch.arange(c), 0, 0] = 1.0  # beta[c] = x[c]
        if entry == "mix":
            wd.inputs = {"in0": x, "in1": zc, "w": wmix}
        else:
            cin = a.cin
            assert cin >= c
            hid = torch.ones(B, cin, H, W)
            hid[:, :c] = zc
            w2 = torch.zeros(c, cin, 3, 3)
            w2[torch.arange(c), torch.arange(c), 1, 1] = 1.0  # z[c] = hid[c]
            wd.inputs = {"hid": hid, "x": x, "w2": w2, "wmix": wmix}
        wd.x64, wd.z64 = d(x), d(zc)
        wd.want64 = wd.x64 + 0.5 * torch.sigmoid(wd.x64) * (wd.z64 - wd.x64)
        wd.scale64 = wd.x64.abs() + (wd.z64 - wd.x64).abs()
        wd.may_flush, wd.flushed64 = 0.5 * torch.sigmoid(wd.x64) < RCP_MIN * (1 + REL), wd.x64
        wd.read = x
    op_ref.check_shapes(entry, args, wd.inputs)
    return wd


def window(w: Win) -> Window:
    return _cached_window(w.entry, w.args, w.dt)
