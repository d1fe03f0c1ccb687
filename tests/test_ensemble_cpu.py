"""The dihedral transforms and the self-ensemble without a GPU: mz_dihedral_inverse against the numpy composition of the transforms, the
chunk planner of upscale_ensemble, every refused argument of mz_dihedral / mz_ensemble_add / mz_ensemble_finish (refused before anything
touches a device), the accumulator's size, and the Python layer's refusals."""

import re
from ctypes import byref, c_int32, c_int64, c_size_t, c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

from ultrazoom_amd import _ffi
from ultrazoom_amd.ensemble import DEFAULT_WORKSPACE_BYTES, plan_chunks

REPO = Path(__file__).resolve().parent.parent
B, H, W = 2, 48, 64
FAKE, FAKE2 = 0x1000000, 0x40000000  # never dereferenced: validation comes first; far enough apart for every shape used here


def T(a, k):
    """Orientation k of a numpy [H, W] array, as the header states it."""
    if k & 2:
        a = a[::-1, :]
    if k & 1:
        a = a[:, ::-1]
    if k & 4:
        a = a.T
    return a


# ---- mz_dihedral_inverse ---------------------------------------------------------------------------------------------------------
def test_inverse_undoes_every_orientation():
    a = np.arange(5 * 7).reshape(5, 7)
    for k in range(8):
        inv = _ffi.dihedral_inverse(k)
        assert 0 <= inv <= 7 and _ffi.dihedral_inverse(inv) == k
        assert inv == (k if k < 4 else 4 | ((k & 1) << 1) | ((k & 2) >> 1))
        assert np.array_equal(T(T(a, k), inv), a), k
        assert T(a, k).shape == ((7, 5) if k & 4 else (5, 7))
    assert [_ffi.dihedral_inverse(k) for k in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    for bad in (-1, 8, 1 << 30, -(1 << 31)):
        assert _ffi.dihedral_inverse(bad) < 0, bad


def test_the_eight_transforms_are_a_group():
    """All different, and closed under composition: T(T(a, j), k) is one of the eight again; the inverse is the one that composes to 0."""
    a = np.arange(4 * 4).reshape(4, 4)  # square: every composition has the one shape
    images = [T(a, k).tobytes() for k in range(8)]
    assert len(set(images)) == 8
    for j in range(8):
        row = [images.index(T(T(a, j), k).tobytes()) for k in range(8)]  # (ValueError: not closed)
        assert sorted(row) == list(range(8)), (j, row)
        assert row[_ffi.dihedral_inverse(j)] == 0, (j, row)


# ---- the chunk planner -----------------------------------------------------------------------------------------------------------
def test_plan_chunks_covers_the_batch_within_the_budget():
    per = 3 * 96 * 128 * (4 + 2)
    assert plan_chunks(5, 96, 128, 2, DEFAULT_WORKSPACE_BYTES) == [(0, 5)]
    assert plan_chunks(5, 96, 128, 2, per) == [(b, 1) for b in range(5)]
    assert plan_chunks(5, 96, 128, 2, 2 * per + per - 1) == [(0, 2), (2, 2), (4, 1)]
    assert plan_chunks(5, 96, 128, 2, 5 * per) == [(0, 5)]
    assert plan_chunks(1, 1, 1, 1, 15) == [(0, 1)]
    # 16 x 8K in bfloat16 under the default budget: 597 MB an image, seven at a time
    chunks = plan_chunks(16, 4320, 7680, 2, DEFAULT_WORKSPACE_BYTES)
    assert chunks == [(0, 7), (7, 7), (14, 2)]
    for elem_bytes in (1, 2, 4):
        for budget in (3 * 40 * 56 * (4 + elem_bytes) * m + extra for m in (1, 2, 3, 7, 9) for extra in (0, 5)):
            got = plan_chunks(9, 40, 56, elem_bytes, budget)
            assert [b for b, _ in got] == [sum(n for _, n in got[:i]) for i in range(len(got))] and sum(n for _, n in got) == 9
            assert all(1 <= n <= got[0][1] and n * 3 * 40 * 56 * (4 + elem_bytes) <= budget for _, n in got), got
    with pytest.raises(ValueError, match="below"):
        plan_chunks(5, 96, 128, 2, per - 1)
    for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 8, 3)):
        with pytest.raises(ValueError):
            plan_chunks(*bad, DEFAULT_WORKSPACE_BYTES)


# ---- refusals of the C entries ---------------------------------------------------------------------------------------------------
def dense(h, w):
    return (3 * h * w, h * w, w, 1)


def view(data=FAKE, strides=None, h=H, w=W):
    return _ffi.MzImageView(c_void_p(data), (c_int64 * 4)(*(strides or dense(h, w))))


def last_error():
    return _ffi.lib().mz_last_error().decode()


def call_dihedral(x="dense", out="dense", elem=0, batch=B, h=H, w=W, k=5):
    ho, wo = (w, h) if k & 4 else (h, w)
    x = view() if x == "dense" else x
    out = view(data=FAKE2, h=ho, w=wo) if out == "dense" else out
    code = _ffi.lib().mz_dihedral(byref(x) if x is not None else None, byref(out) if out is not None else None, elem, batch, h, w, k, None)
    return code, last_error()


def call_add(y="dense", elem=0, batch=B, h=H, w=W, k=5, first=1, ws=FAKE2, ws_bytes=1 << 40):
    hy, wy = (w, h) if k & 4 else (h, w)
    y = view(h=hy, w=wy) if y == "dense" else y
    code = _ffi.lib().mz_ensemble_add(byref(y) if y is not None else None, elem, batch, h, w, k, first, c_void_p(ws) if ws else None, ws_bytes, None)
    return code, last_error()


def call_finish(out="dense", elem=0, batch=B, h=H, w=W, n=8, window=None, ws=FAKE2, ws_bytes=1 << 40):
    out = view() if out == "dense" else out
    win = (c_int32 * 4)(*window) if window is not None else None
    code = _ffi.lib().mz_ensemble_finish(byref(out) if out is not None else None, elem, batch, h, w, n, 1, win, c_void_p(ws) if ws else None,
                                         ws_bytes, None)
    return code, last_error()


D = dense(H, W)
DT = dense(W, H)  # the output of a transposing orientation
DIHEDRAL_REFUSED = {
    "null input view": dict(x=None),
    "null output view": dict(out=None),
    "null input data": dict(x=view(data=None)),
    "null output data": dict(out=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "k -1": dict(k=-1),
    "k 8": dict(k=8),
    "no images": dict(batch=0),
    "65536 images": dict(batch=65536),
    "no rows": dict(h=0),
    "negative width": dict(w=-3),
    "a side beyond 2^28": dict(w=(1 << 28) + 1),
    "output channel stride 0": dict(out=view(FAKE2, (DT[0], 0, DT[2], 1))),
    "output row stride 0": dict(out=view(FAKE2, (DT[0], DT[1], 0, 1))),
    "output column stride 0": dict(out=view(FAKE2, (DT[0], DT[1], DT[2], 0))),
    "output image stride 0 with two images": dict(out=view(FAKE2, (0,) + DT[1:])),
    "in place": dict(out=view(FAKE, DT)),
    "out begins inside x": dict(out=view(FAKE + 4 * (B * 3 * H * W - 1), DT)),
    "out ends inside x": dict(out=view(FAKE - 4 * (B * 3 * H * W - 1), DT)),
    "x inside a strided out": dict(out=view(FAKE - 64, tuple(2 * s for s in DT))),
    "a byte range beyond 63 bits": dict(x=view(strides=((1 << 62), D[1], D[2], 1))),
}
ADD_REFUSED = {
    "null view": dict(y=None),
    "null data": dict(y=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "k -1": dict(k=-1),
    "k 8": dict(k=8),
    "no images": dict(batch=0),
    "65536 images": dict(batch=65536),
    "no columns": dict(w=0),
    "a side beyond 2^28": dict(h=(1 << 28) + 1),
    "y inside the accumulator": dict(y=view(data=FAKE2 + 64, h=W, w=H)),
}
FINISH_REFUSED = {
    "null view": dict(out=None),
    "null data": dict(out=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "n 0": dict(n=0),
    "n 3": dict(n=3),
    "n 16": dict(n=16),
    "n -8": dict(n=-8),
    "no images": dict(batch=0),
    "65536 images": dict(batch=65536),
    "no rows": dict(h=0),
    "channel stride 0": dict(out=view(FAKE, (D[0], 0, D[2], 1))),
    "row stride 0": dict(out=view(FAKE, (D[0], D[1], 0, 1))),
    "column stride 0": dict(out=view(FAKE, (D[0], D[1], D[2], 0))),
    "image stride 0 with two images": dict(out=view(FAKE, (0,) + D[1:])),
    "empty window": dict(window=(0, 0, 0, 5)),
    "window with a negative corner": dict(window=(-1, 0, 4, 4)),
    "window beyond the last row": dict(window=(H - 3, 0, 4, 4)),
    "window beyond the last column": dict(window=(0, W - 3, 4, 4)),
    "out inside the accumulator": dict(out=view(data=FAKE2 + 64)),
}
CASES = ([(call_dihedral, "dihedral", n, a) for n, a in DIHEDRAL_REFUSED.items()] + [(call_add, "add", n, a) for n, a in ADD_REFUSED.items()] +
         [(call_finish, "finish", n, a) for n, a in FINISH_REFUSED.items()])


@pytest.mark.parametrize("call, entry, name, args", CASES, ids=[f"{e}: {n}" for _, e, n, _ in CASES])
def test_bad_arguments_are_refused_before_the_gpu(call, entry, name, args):
    code, msg = call(**args)
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (entry, name, code, msg)
    assert msg, (entry, name)


def test_null_and_short_workspaces_are_refused():
    need = 12 * B * H * W
    assert _ffi.ensemble_workspace_bytes(B, H, W) == need
    for call in (call_add, call_finish):
        for args in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None, ws_bytes=0)):
            code, msg = call(**args)
            assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL and "workspace too small" in msg, (call.__name__, args, code, msg)


def test_what_validation_lets_through_stops_at_the_workspace():
    """Still without a GPU call: every orientation, element type and n, signed and zero input strides, a window, one image with an image
    stride of 0."""
    for k in range(8):
        for elem in range(4):
            assert call_add(k=k, elem=elem, ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL, (k, elem)
    assert call_add(y=view(strides=(0, 0, 0, 0)), ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL
    assert call_add(y=view(data=FAKE + 4 * (3 * H * W - 1), strides=(D[0], -D[1], -D[2], -1)), k=0, ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL
    for n in (1, 2, 4, 8):
        for elem in range(4):
            assert call_finish(n=n, elem=elem, ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL, (n, elem)
    assert call_finish(window=(H - 4, W - 4, 4, 4), ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL
    assert call_finish(batch=1, out=view(FAKE, (0,) + D[1:]), ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL
    assert call_finish(batch=65535, ws_bytes=8)[0] == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL


def test_workspace_bytes_is_the_float32_accumulator():
    n = c_size_t()
    wsb = _ffi.lib().mz_ensemble_workspace_bytes
    for b, h, w in ((1, 1, 1), (2, 48, 64), (16, 4320, 7680), (1, 37000, 39000), (65535, 1 << 14, 1 << 14)):
        assert wsb(b, h, w, byref(n)) == 0 and n.value == 12 * b * h * w
    for bad in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, -1), (1, (1 << 28) + 1, 8), (65535, 1 << 28, 1 << 28)):
        assert wsb(*bad, byref(n)) == _ffi.MZ_ERR_INVALID_ARGUMENT, bad
    assert wsb(1, 8, 8, None) == _ffi.MZ_ERR_INVALID_ARGUMENT


def test_header_declares_the_entries():
    text = (REPO / "include" / "mewzoom_hip.h").read_text()
    assert re.search(r"\bint mz_dihedral_inverse\(int k\);", text)
    assert re.search(r"\bint mz_dihedral\(const mz_image_view\* x, const mz_image_view\* out, int elem, int B, int H, int W, int k, void\* hip_stream\);", text)
    assert re.search(r"\bint mz_ensemble_workspace_bytes\(int B, int H, int W, size_t\* bytes\);", text)
    assert re.search(r"\bint mz_ensemble_add\(const mz_image_view\* y, int elem, int B, int H, int W, int k, int first,", text)
    assert re.search(r"\bint mz_ensemble_finish\(const mz_image_view\* out, int elem, int B, int H, int W, int n, int clamp,", text)
    units = (REPO / "ultrazoom_amd" / "csrc" / "units.sh").read_text()
    assert re.search(r"kernel_units=\([^)]*\bmz_dihedral\b", units)
    kernel = (REPO / "ultrazoom_amd" / "csrc" / "mz_dihedral.h").read_text()
    tile = int(re.search(r"constexpr int kDihedralTile = (\d+);", kernel).group(1))
    assert tile == 64 and re.search(r"constexpr int kDihedralPitch = kDihedralTile \+ 1;", kernel)  # an odd dword pitch
    assert (tile + 1) * tile * 4 <= 64 * 1024


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_python_layer():
    import ultrazoom_amd
    from golden_util import GoldenCase
    from ultrazoom_amd import MewZoom, dihedral, dihedral_inverse, upscale_ensemble
    from ultrazoom_amd.synth import synth_image

    assert {"dihedral", "dihedral_inverse", "upscale_ensemble"} <= set(ultrazoom_amd.__all__)
    assert [dihedral_inverse(k) for k in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    with pytest.raises(ValueError, match="0..7"):
        dihedral_inverse(8)
    x = synth_image(1, 24, 40, seed=1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        dihedral(x, 3)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        dihedral(x[0], 3)
    with pytest.raises(TypeError, match="unsupported dtype"):
        dihedral(x.double(), 3)
    case = GoldenCase("g1_2x_c16")
    m = MewZoom(**case.config).eval()
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.upscale_ensemble(x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        upscale_ensemble(m, (x * 255).to(torch.uint8), n=2)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m.upscale_ensemble(x[:, :2])


def test_evaluate_refuses_an_ensemble_that_is_no_subgroup():
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr

    class Model:
        upscale_ratio = 2

        def upscale(self, x):
            raise AssertionError("not reached")

    for bad in (0, 3, 16):
        with pytest.raises(ValueError, match="ensemble"):
            evaluate(Model(), [], ensemble=bad)
        with pytest.raises(ValueError, match="ensemble"):
            evaluate_hr(Model(), [], ensemble=bad)
    assert evaluate(Model(), [], ensemble=1)["images"] == 0
