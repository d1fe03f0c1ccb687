"""The degradation chain without a GPU: the Philox generator (three statements of it: the library's host function, the Python one of
`Degradation.sample`, the numpy checker) against the published known-answer vectors, the moments of the checker's normal numbers,
`Degradation.sample`, the quantisation tables, the numpy JPEG model (tests/degrade_ref.py) against a real codec's output
(tests/golden/d1_jpeg_codec.npz: Pillow / libjpeg-turbo), the seeds of tests/test_degrade_gpu.py, and every refused argument of the
three C entries (refused before anything touches a device)."""

import json
import math
import re
from ctypes import byref, c_int64, c_size_t, c_void_p
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import degrade_ref as R
from ultrazoom_amd import _ffi
from ultrazoom_amd.degrade import Degradation, philox4x32_10
from ultrazoom_amd.synth import synth_image

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden"
FAKE, FAKE2 = 0x10000, 0x40000000  # never dereferenced: validation comes first
B, H, W = 2, 37, 45

# Random123's kat_vectors, philox4x32 10: counter and key all zero, all ones, and the digits of pi
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("counter, key, want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers_in_all_three_statements(counter, key, want):
    assert tuple(philox4x32_10(counter, key)) == want
    assert tuple(_ffi.philox(counter, key)) == want
    assert tuple(int(v) for v in R.philox(*counter, *key)) == want


def test_noise_moments_over_a_million_samples():
    """Standard errors at n = 1e6: mean 1e-3, variance 1.4e-3, skewness 2.4e-3, excess kurtosis 4.9e-3: gates at five of them"""
    n = R.normal_ref(1_000_000, seed=7, stream=3)
    mean, var = float(n.mean()), float(n.var())
    z = (n - mean) / math.sqrt(var)
    skew, kurt = float((z**3).mean()), float((z**4).mean()) - 3.0
    print(f"mean {mean:.2e} var {var:.5f} skew {skew:.2e} excess kurtosis {kurt:.2e} max |n| {float(np.abs(n).max()):.2f}")
    assert abs(mean) <= 5e-3 and abs(var - 1.0) <= 7e-3 and abs(skew) <= 1.2e-2 and abs(kurt) <= 2.5e-2
    assert 4.5 < float(np.abs(n).max()) < 6.7  # sqrt(-2 ln(0.5 / 2^32)) = 6.66 bounds it
    other = R.normal_ref(1000, seed=7, stream=4)
    assert abs(float(np.corrcoef(n[:1000], other)[0, 1])) < 0.15 and not np.array_equal(n[:1000], other)


def test_sample_is_reproducible_and_targets_are_normalised():
    d = Degradation(seed=11)
    rows = d.sample(64, index=5)
    assert rows == d.sample(64, index=5) and rows[3:10] == d.sample(7, index=8)  # an image's draw depends on its index alone
    assert rows != Degradation(seed=12).sample(64, index=5)
    for name, k in (("blur", 0), ("noise", 1), ("compression", 2)):
        lo, hi = getattr(d, name)
        vals = [r[k] for r in rows]
        assert all(lo < v < hi for v in vals) and max(vals) - min(vals) > 0.8 * (hi - lo), name
    assert (d.blur, d.noise, d.compression, d.filter) == ((0.0, 1.0), (0.0, 0.1), (0.0, 0.8), "bicubic")
    narrow = Degradation(blur=(0.5, 1.5), noise=(0.02, 0.04), compression=(0.1, 0.3), seed=11)
    got, base = narrow.sample(64, 5), d.targets(rows)
    for t, t0, r in zip(narrow.targets(got), base, got):
        assert all(abs(a - b) <= 1e-12 for a, b in zip(t, t0))  # the same uniforms, whatever the ranges
        assert abs(t[0] - (r[0] - 0.5) / 1.0) <= 1e-15 and abs(t[2] - (r[2] - 0.1) / 0.2) <= 1e-15  # data.py:150-162
    # the draw is the first three words of the block (index, stream 2^64 - 1), key = seed
    u = philox4x32_10((5, 0, 0xFFFFFFFF, 0xFFFFFFFF), (11, 0))
    assert rows[0] == tuple(lo + (hi - lo) * (u[k] + 0.5) / 2**32 for k, (lo, hi) in enumerate(((0.0, 1.0), (0.0, 0.1), (0.0, 0.8))))
    with pytest.raises(ValueError, match="filter"):
        Degradation(filter="nearest")
    with pytest.raises(ValueError, match="range"):
        Degradation(noise=(0.1, 0.1))


def test_quantisation_tables():
    for q in (1, 20, 50, 90, 100):
        luma, chroma = _ffi.jpeg_qtable(q)
        wl, wc = R.qtables(q)
        assert luma == wl.flatten().tolist() and chroma == wc.flatten().tolist(), q
    assert _ffi.jpeg_qtable(100) == ([1] * 64, [1] * 64)
    assert _ffi.jpeg_qtable(50) == (R.K1.flatten().tolist(), R.K2.flatten().tolist())
    luma1, chroma1 = _ffi.jpeg_qtable(1)
    assert set(luma1) == {255} and set(chroma1) == {255}  # scale 5000: everything clamps
    assert _ffi.jpeg_qtable(20)[0][:3] == [40, 28, 25]  # (16, 11, 10) * 250 + 50) / 100


def test_blur_weights_of_the_library_are_the_checkers():
    for sigma in (0.2, 0.34, 1.0, 1.7, 2.5, 5.3):
        got, want = _ffi.blur_weights(sigma), R.blur_weights(sigma).tolist()
        assert len(got) == 2 * int(3 * sigma) + 1 == len(want)
        assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-15 and abs(math.fsum(got) - 1.0) <= 1e-15
    assert _ffi.blur_weights(0.2) == [1.0] and _ffi.blur_weights(0.0) == [1.0]
    with pytest.raises(_ffi.MewZoomHipError):
        _ffi.blur_weights(5.34)


def test_a_float_quotient_rounds_once():
    """v / 255 as the kernel stores it in a 16-bit type ((float)v / 255.0f, then one conversion) is the correctly rounded v / 255: no
    float32 quotient lies on a tie of the 16-bit grid, so rounding twice cannot differ from rounding once."""
    v = torch.arange(256, dtype=torch.float32) / 255.0
    for dtype, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        got = v.to(dtype).double().tolist()
        for k, g in enumerate(got):
            exact = Fraction(k, 255)
            if k == 0:
                assert g == 0.0
                continue
            e = math.floor(math.log2(exact))
            ulp = Fraction(2) ** (e - bits + 1)
            assert abs(Fraction(g) - exact) < ulp / 2, (dtype, k)  # strictly nearest: no tie


@pytest.fixture(scope="module")
def codec():
    return np.load(GOLDEN / "d1_jpeg_codec.npz")


def test_the_jpeg_model_against_a_real_codec(codec):
    """Measures the numpy model against Pillow's output and writes tests/golden/degrade_codec.json, the record the GPU test reads.  The
    model is float64 and exact where libjpeg's DCT is a scaled-integer one, so they differ by rounding: the figures are recorded, and
    held only to the loose bounds that tell a model of the codec from something else (mean-abs under 1 LSB, PSNR over 40 dB)."""
    record = {}
    for i in range(3):
        x = torch.from_numpy(codec[f"in_{i}"])[None]
        for q in (20, 50, 90, 100):
            out, _, share = R.jpeg_ref(x, q)
            want = codec[f"out_{i}_q{q}"].astype(np.int64)
            diff = np.abs(out[0] - want)
            mse = float((diff.astype(np.float64) ** 2).mean())
            record[f"{i}_q{q}"] = {"shape": list(want.shape[1:]), "mean_abs": round(float(diff.mean()), 6), "max_abs": int(diff.max()),
                                   "psnr": round(10 * math.log10(255.0**2 / mse), 4), "near_tie_share": share}
            print(f"image {i} q {q}: {record[f'{i}_q{q}']}")
            assert float(diff.mean()) < 1.0 and record[f"{i}_q{q}"]["psnr"] > 40.0, (i, q)
            # and the codec really compressed: its output is not its input
            assert q == 100 or float(np.abs(want - codec[f"in_{i}"].astype(np.int64)).mean()) > 2 * float(diff.mean())
    path = GOLDEN / "degrade_codec.json"
    text = json.dumps(record, indent=1, sort_keys=True) + "\n"
    if not path.exists() or path.read_text() != text:
        path.write_text(text)
    assert json.loads(path.read_text()) == record


def test_the_gpu_tests_seeds_stay_under_their_caps():
    """What tests/test_degrade_gpu.py assumes of its inputs, checked with the checker alone: JPEG near-tie blocks under 1 % per case
    (expected: about 1e-4), and for uint8 noise fewer than 0.1 % of the elements within 1e-6 of a rounding tie."""
    for shape in R.SHAPES:
        for q in R.QUALITIES:
            for dt in ("u8", "f32"):
                _, _, share = R.jpeg_ref(R.image(R.BATCH, *shape, dt), q)
                assert share < 0.01, (shape, q, dt, share)
    for shape in R.SHAPES:
        for sigma in R.NOISE_SIGMAS:
            scaled = R.noise_ref(R.image(R.BATCH, *shape, "u8"), sigma, R.SEED, R.OFFSET) * 255
            near = ((scaled - torch.floor(scaled)) - 0.5).abs() <= 1e-6
            assert float(near.double().mean()) < 1e-3, (shape, sigma)


def test_a_constant_image_survives_quality_100():
    for v in (0, 77, 128, 255):
        x = torch.full((1, 3, 17, 33), v, dtype=torch.uint8)
        out, unsure, _ = R.jpeg_ref(x, 100)
        assert not unsure.any() and np.abs(out - v).max() <= 1  # grey: Y = v, chroma 128; the colour matrices round trip within 1


# ---- the C entries refuse what the Python layer refuses -----------------------------------------------------------------------------------
def view(data=FAKE, strides=None):
    return _ffi.MzImageView(c_void_p(data), (c_int64 * 4)(*(strides or (3 * H * W, H * W, W, 1))))


def call(entry, x="dense", out="dense", elem=0, batch=B, h=H, w=W, sigma=1.0, quality=50, ws=FAKE, ws_bytes=1 << 40):
    x = view() if x == "dense" else x
    out = view(FAKE2) if out == "dense" else out
    xp, op = (byref(x) if x is not None else None), (byref(out) if out is not None else None)
    lib = _ffi.lib()
    if entry == "blur":
        code = lib.mz_blur(xp, op, elem, batch, h, w, sigma, None)
    elif entry == "noise":
        code = lib.mz_noise(xp, op, elem, batch, h, w, sigma, 1, 0, None)
    else:
        code = lib.mz_jpeg(xp, op, elem, batch, h, w, quality, c_void_p(ws) if ws else None, ws_bytes, None)
    return code, lib.mz_last_error().decode()


DENSE = (3 * H * W, H * W, W, 1)
COMMON = {
    "null input view": dict(x=None),
    "null output view": dict(out=None),
    "null input data": dict(x=view(data=None)),
    "null output data": dict(out=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "no images": dict(batch=0),
    "65536 images": dict(batch=65536),
    "no rows": dict(h=0),
    "negative width": dict(w=-3),
    "output channel stride 0": dict(out=view(FAKE2, (DENSE[0], 0, W, 1))),
    "output row stride 0": dict(out=view(FAKE2, (DENSE[0], DENSE[1], 0, 1))),
    "output column stride 0": dict(out=view(FAKE2, (DENSE[0], DENSE[1], W, 0))),
    "output image stride 0 with two images": dict(out=view(FAKE2, (0,) + DENSE[1:])),
    "out overlaps x": dict(out=view(FAKE + 4 * W)),
}
OWN = {
    "blur": {"negative sigma": dict(sigma=-0.5), "nan sigma": dict(sigma=float("nan")), "half 16": dict(sigma=16 / 3 + 1e-9),
             "5x5 with sigma 1.7": dict(h=5, w=5, sigma=1.7), "a row of 3 with sigma 1": dict(h=3, sigma=1.0),
             "in place": dict(out=view(FAKE))},
    "noise": {"negative sigma": dict(sigma=-1e-3), "nan sigma": dict(sigma=float("nan")), "infinite sigma": dict(sigma=float("inf"))},
    "jpeg": {"quality 0": dict(quality=0), "quality 101": dict(quality=101), "in place": dict(out=view(FAKE))},
}
REFUSED = [(e, n, a) for e in ("blur", "noise", "jpeg") for n, a in list(COMMON.items()) + list(OWN[e].items())]


@pytest.mark.parametrize("entry, name, args", REFUSED, ids=[f"{e}: {n}" for e, n, _ in REFUSED])
def test_bad_arguments_are_refused_before_the_gpu(entry, name, args):
    code, msg = call(entry, **args)
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (entry, name, code, msg)
    assert msg, name


def test_what_validation_lets_through_stops_at_the_workspace():
    for args in (dict(), dict(elem=1), dict(elem=2), dict(elem=3), dict(quality=1), dict(quality=100), dict(batch=65535, out=view(FAKE2 * 8)),
                 dict(x=view(FAKE + 8 * H * W, (3 * H * W, -H * W, W, 1))), dict(x=view(strides=(0, 0, 0, 0))), dict(h=1, w=1, batch=1)):
        code, msg = call("jpeg", ws_bytes=8, **args)
        assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL and "workspace too small" in msg, (args, code, msg)
    assert call("jpeg", ws=None)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL


def test_jpeg_workspace_holds_the_decoded_planes():
    for b, h, w in ((1, 16, 16), (2, 17, 33), (3, 37, 45), (16, 1080, 1920)):
        n = _ffi.jpeg_workspace_bytes(b, h, w)
        planes = b * (-(-h // 16) * 16) * (-(-w // 16) * 16) * 3 // 2
        assert planes <= n <= planes + 512 and n == _ffi.jpeg_workspace_bytes(b, h, w)
    size = c_size_t()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (65536, 8, 8)):
        assert _ffi.lib().mz_jpeg_workspace_bytes(*bad, byref(size)) == _ffi.MZ_ERR_INVALID_ARGUMENT, bad
    assert _ffi.lib().mz_jpeg_workspace_bytes(1, 8, 8, None) == _ffi.MZ_ERR_INVALID_ARGUMENT


def test_header_declares_the_entries():
    text = (REPO / "include" / "mewzoom_hip.h").read_text()
    for decl in (r"int mz_blur\(const mz_image_view\* x, const mz_image_view\* out, int elem, int B, int H, int W, double sigma, void\* hip_stream\);",
                 r"int mz_noise\(const mz_image_view\* x, const mz_image_view\* out, int elem, int B, int H, int W, double sigma, uint64_t seed,",
                 r"int mz_jpeg_workspace_bytes\(int B, int H, int W, size_t\* bytes\);",
                 r"int mz_jpeg\(const mz_image_view\* x, const mz_image_view\* out, int elem, int B, int H, int W, int quality, void\* workspace,"):
        assert re.search(decl, text), decl
    kernel = (REPO / "ultrazoom_amd" / "csrc" / "mz_degrade.h").read_text()
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert word in kernel, word


def test_refusals_of_the_python_layer():
    from ultrazoom_amd.degrade import gaussian_blur, gaussian_noise, jpeg
    from ultrazoom_amd.evaluate import evaluate_hr

    x = synth_image(2, 24, 40, seed=1)
    for fn, args, kw in ((gaussian_blur, (1.0,), {}), (gaussian_noise, (0.1,), dict(seed=1)), (jpeg, (50,), {})):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(x, *args, **kw)
        with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
            fn(x[0], *args, **kw)
        with pytest.raises(TypeError, match="unsupported dtype"):
            fn(x.double(), *args, **kw)
    with pytest.raises(RuntimeError, match="MI355X only"):
        Degradation().apply(x, 2)
    with pytest.raises(ValueError, match="backend='hip'"):
        evaluate_hr(object(), [x], degrade=Degradation())
