"""The exact-arithmetic reference of the filtering image operators (tests/image_exact.py) without a GPU: its fma against rational arithmetic
and libm, its taps against the library's bit for bit, the restatement against torch inside the gates the suite had before, the uint8 store
rule fused and unfused, and its discriminating power: every case of tests/test_image_exact_gpu.py against five deliberately wrong
restatements (EXPERIMENTS.md section 22 holds the printed counts and the reference's times)."""

import math
import random
import time
from collections import defaultdict
from ctypes import CDLL, c_double

import numpy as np
import pytest
import torch

import degrade_ref
import image_exact as ie
import interp_util
import resize_util
from gpu_util import ulp_of
from ultrazoom_amd import _ffi

libm = CDLL("libm.so.6")
libm.fma.restype = c_double
libm.fma.argtypes = [c_double, c_double, c_double]


def same_float(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def hold(triples):
    a, b, c = (np.array(v, dtype=np.float64) for v in zip(*triples))
    got = ie.fma64(a, b, c)
    for (x, y, z), g in zip(triples, got.tolist()):
        exact, lib = ie.fma_exact(x, y, z), libm.fma(x, y, z)
        assert same_float(exact, lib), (x.hex(), y.hex(), z.hex(), exact, lib)
        assert same_float(g, lib), (x.hex(), y.hex(), z.hex(), g, lib)


def test_fma64_on_random_triples():
    """1e5 triples: mantissas of all 53 bits, exponents as the image operators meet them and wider, c near the product and far from it"""
    r = random.Random(5)

    def draw(lo, hi):
        return math.ldexp(r.choice((-1, 1)) * (r.getrandbits(52) | (1 << 52)), r.randint(lo, hi) - 52)

    triples = []
    for n in range(100000):
        a, b = draw(-40, 20), draw(-40, 20)
        kind = n % 4
        c = draw(-80, 40) if kind == 0 else -a * b * (1 + r.randint(-4, 4) * 2.0 ** -r.randint(30, 52)) if kind == 1 else \
            a * b * 2.0 ** r.randint(-60, 60) * r.choice((-1, 1)) if kind == 2 else draw(-1000, 1000)
        triples.append((a, b, c))
    hold(triples)


def test_fma64_on_engineered_triples():
    r = random.Random(6)
    triples = []
    for _ in range(2000):
        a, b = r.uniform(-2, 2), r.uniform(-2, 2)
        triples.append((a, b, -(a * b)))                           # cancels to the product's own rounding error
        triples.append((a, b, -float(np.nextafter(a * b, 4.0))))   # and to one unit beside it
        m = r.getrandbits(52) | (1 << 52)
        triples.append((float(m), 1.0, 0.5))                       # m + 1/2: a tie of float64, even and odd m
        triples.append((float(m), -1.0, -0.5))
        triples.append((float(m | 1), 0.5, 0.0 if m & 2 else 2.0 ** -60))  # an odd product halved: exact; with a crumb beside it
        p, q = (1 << 26) + 2 * r.getrandbits(20) + 1, (1 << 26) + 2 * r.getrandbits(20) + 1
        triples.append((float(p), float(q), 0.0))                  # c = 0: the product of two 27-bit numbers rounded once
        triples.append((float(p), float(q), -0.0))
        triples.append((float(p), float(q), 0.5 * (p * q % 2 + 1)))
        s = math.ldexp(r.uniform(1, 2), -r.randint(500, 540))
        triples.append((s, math.ldexp(r.uniform(-2, 2), -r.randint(520, 560)), math.ldexp(r.uniform(-1, 1), -1070)))  # subnormal results
        triples.append((s, s, -(s * s)))
        triples.append((5e-324, 0.5, 5e-324 * r.randint(0, 3)))
    triples += [(0.0, 3.0, -0.0), (-0.0, 3.0, 0.0), (-0.0, 3.0, -0.0), (0.0, -3.0, -0.0), (1.0, 1.0, -1.0), (-1.0, 1.0, 1.0), (1e308, 10.0, -1e308),
                (1e308, 10.0, -math.inf), (math.inf, 0.0, 1.0), (math.inf, 1.0, -math.inf), (math.nan, 1.0, 1.0), (2.0 ** 600, 2.0 ** 600, -math.inf),
                (2.0 ** 511, 2.0 ** 512, -(2.0 ** 1023)), (1 + 2.0 ** -52, 1.0, 2.0 ** -53), (1 + 2.0 ** -51, 1.0, -(2.0 ** -53))]
    hold(triples)


# ---- the taps ---------------------------------------------------------------------------------------------------------------------------------
def axes_of(op):
    return sorted({(c.shape[0][a], c.shape[1][a], c.how) for c in ie.CASES if c.op == op for a in (0, 1)})


def test_restated_taps_are_the_librarys_bit_for_bit():
    n = 0
    for n_in, n_out, mode in axes_of("interp") + [(a, b, "nearest") for a, b, _ in axes_of("interp")]:
        for i in range(n_out):
            assert _ffi.interp_taps(n_in, n_out, interp_util.MODE[mode], i) == tuple(ie.interp_taps(n_in, n_out, mode, i)), (n_in, n_out, mode, i)
            n += 1
    for n_in, n_out, filt in axes_of("resize"):
        for i in range(n_out):
            assert _ffi.resize_taps(n_in, n_out, resize_util.FILTERS.index(filt), i) == ie.resize_taps(n_in, n_out, filt, i), (n_in, n_out, filt, i)
            n += 1
    for sigma in sorted({c.how for c in ie.CASES if c.op == "blur"}):
        assert _ffi.blur_weights(sigma) == ie.blur_weights(sigma), sigma
        n += 1
    print(n, "tables")
    assert [ie.reflect(i, 5) for i in range(-4, 9)] == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0]


# ---- the same function as torch's -----------------------------------------------------------------------------------------------------------
NOISE_CASES = [c for c in ie.CASES if c.kind == "noise" and not c.via and not c.clamp]


@pytest.mark.parametrize("c", NOISE_CASES, ids=ie.case_id)
def test_the_restatement_is_torchs_function_inside_the_earlier_gates(c):
    for dt in c.dts:
        x = ie.case_input(c, dt)
        want64 = degrade_ref.blur_ref(x, c.how) if c.op == "blur" else (interp_util if c.op == "interp" else resize_util).want64_of(x, c.shape[1], c.how)
        got = ie.case_expected(c, dt).want
        if dt in ("f32", "u8"):
            resize_util.assert_within_gate(got, want64, dt, f"{ie.case_id(c)} {dt}")
        else:  # one ulp of the stored type at the float64 value, which below interp_util.NOISE_FLOOR is torch's own rounding noise
            diff = (got.double() - want64).abs()
            assert bool((diff <= ulp_of(want64, dt).double() + interp_util.NOISE_FLOOR).all()), (ie.case_id(c), dt, float(diff.max()))


# ---- the uint8 store rule -----------------------------------------------------------------------------------------------------------------
def test_uint8_store_rule_fused_and_unfused_give_the_same_bytes():
    """u8_of_unit() (mz_view.h) is written v * 255.0f + 0.5f; the compiler is free to fuse it.  Every float32 within 64 ulps of each of
    the 255 thresholds (k - 0.5) / 255, and every value the uint8 cases of the GPU test hand to it, gives the same byte both ways."""
    k = np.arange(1, 256, dtype=np.float64)
    centre = ((k - 0.5) / 255.0).astype(np.float32).view(np.int32)
    v = (centre[:, None] + np.arange(-64, 65, dtype=np.int32)[None, :]).reshape(-1).view(np.float32)
    assert v.size == 255 * 129 == 32895
    fused, unfused = ie.u8_of_unit_fused(v), ie.u8_of_unit(v)
    assert (fused == unfused).all()
    assert len(set(unfused.tolist())) == 256  # the sweep crosses every threshold
    edge = np.array([0.0, -0.0, 1.0, -1.0, 2.0, 1e-30, -1e-30, np.float32(1.0) - np.float32(2.0 ** -24), 0.00196, 0.00197], dtype=np.float32)
    assert (ie.u8_of_unit_fused(edge) == ie.u8_of_unit(edge)).all()
    n = 0
    for c in ie.CASES:
        if c.op != "interp" and "u8" in c.dts:
            fed = ie.case_expected(c, "u8").last.astype(np.float32).reshape(-1)
            assert (ie.u8_of_unit_fused(fed) == ie.u8_of_unit(fed)).all(), ie.case_id(c)
            n += fed.size
    print(n, "values of the uint8 cases")
    assert n > 100000


# ---- what the inputs reach ------------------------------------------------------------------------------------------------------------------
SMALLEST_NORMAL = {"f32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -14}


def test_number_range_inputs_reach_their_range():
    negative_zero = defaultdict(int)
    for c, dt in ie.PAIRS:
        if c.kind in ie.SUBNORMAL:
            x, want = ie.case_input(c, dt), ie.case_expected(c, dt).want
            assert float(x.double().abs().max()) < SMALLEST_NORMAL[dt] and float(want.double().abs().max()) < SMALLEST_NORMAL[dt], (ie.case_id(c), dt)
            # (a few units of the smallest subnormal, averaged by a shrinking filter, mostly round to a zero: those cases are after its sign)
            assert int((want != 0).sum()) > want.numel() // (2 if c.kind == "sub_hi" else 8), (ie.case_id(c), dt)
            negative_zero[c.op, dt] += int(((want == 0) & torch.signbit(want)).sum())
        elif c.kind == "over":
            want = ie.case_expected(c, dt).want
            n = int(want.isinf().sum())
            print(f"{ie.case_id(c)} {dt}: {n} of {want.numel()} results are infinite")
            assert bool(ie.case_input(c, dt).isfinite().all()) and 1 <= n < want.numel() // 2 and not bool(want.isnan().any())
    print({f"{op} {dt}": n for (op, dt), n in negative_zero.items()})
    assert len(negative_zero) == 9 and min(negative_zero.values()) >= 1, dict(negative_zero)


@pytest.mark.parametrize("c", [c for c in ie.CASES if c.kind == "nonfinite"], ids=ie.case_id)
def test_non_finite_pixels_reach_exactly_the_outputs_that_name_them(c):
    tx = ie.horizontal_table(c)
    ty = ie.blur_table(c.shape[0], c.how) if c.op == "blur" else (ie.interp_table if c.op == "interp" else ie.resize_table)(c.shape[0][0], c.shape[1][0], c.how)
    H, W = ie.in_shape(c)
    for dt in c.dts:
        x = ie.case_input(c, dt)
        want = ie.case_expected(c, dt).want
        plain = x.clone()
        plain[0, 0, H // 3, W // 2] = plain[1, 1, H // 2, W // 3] = 0.5
        rest = ie.expected(c, dt, plain)
        named = torch.zeros(want.shape, dtype=torch.bool)
        for b, ch, y, xx in ((0, 0, H // 3, W // 2), (1, 1, H // 2, W // 3)):
            rows = torch.from_numpy(((ty.idx == y) & ty.mask).any(axis=1))
            cols = torch.from_numpy(((tx.idx == xx) & tx.mask).any(axis=1))
            named[b, ch] = rows[:, None] & cols[None, :]
        assert 2 <= int(named.sum()) < named.numel() // 4
        assert bool((~want[named].isfinite()).all()) and bool(want[0, 0].isinf().any() | want[0, 0].isnan().any()) and bool(want[1, 1].isnan().any())
        assert bool(ie.same_bits(want, rest)[~named].all())


# ---- discriminating power ---------------------------------------------------------------------------------------------------------------------
def test_every_case_against_the_wrong_restatements():
    """Prints, for every case and type, the reference's wall time and in how many elements each wrong restatement departs from it.
    float32 storage: every applicable wrong restatement departs in at least one case of every (operator, mode or filter).  The planted
    cases part truncation and the other tie rule from the reference for bf16, f16 and uint8."""
    names = list(ie.WRONG)
    separated = defaultdict(lambda: defaultdict(int))
    slow = []
    for c, dt in ie.PAIRS:
        x = ie.case_input(c, dt)
        t0 = time.perf_counter()
        want = ie.expected(c, dt, x)
        took = time.perf_counter() - t0
        if took > 5.0:
            slow.append((ie.pair_id((c, dt)), took))
        counts = {name: ie.differs(c, dt, x, ar, want) if ie.applicable(c, dt, name) else None for name, ar in ie.WRONG.items()}
        counts["other tie rule"] = ie.differs(c, dt, x, ie.OTHER_TIE, want)
        print(f"{ie.pair_id((c, dt))}: reference {took:.2f} s, {want.numel()} elements; " + ", ".join(f"{k} {v}" for k, v in counts.items()))
        if dt == "f32" and not ie.one_by_one(c):
            how = "sigma" if c.op == "blur" else c.how
            for name in names:
                separated[c.op, how][name] += counts[name] or 0
        if c.kind == "ties":
            even, odd, beside = ie.tie_census(c, dt, x)
            print(f"    exact ties below an even / odd neighbour {even} / {odd}, elements beside a tie {beside}")
            assert min(even, odd) >= ie.MIN_TIES and beside >= ie.MIN_TIES, (ie.case_id(c), dt, even, odd, beside)
            if dt != "f32":
                assert counts["final truncation"] >= 1 and counts["other tie rule"] >= 1, (ie.case_id(c), dt, counts)
    assert not slow, slow
    print({f"{op} {how}": dict(v) for (op, how), v in separated.items()})
    assert sorted(separated) == [("blur", "sigma"), ("interp", "bicubic"), ("interp", "bilinear"), ("resize", "bicubic"), ("resize", "bilinear")]
    for key, v in separated.items():
        for name in names:
            if key[0] == "interp" or name != "intermediate in the stored type":
                assert v[name] >= 1, (key, name)
