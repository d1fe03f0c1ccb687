"""The refusals every image-view entry shares (ultrazoom_amd/csrc/mz_view_check.h; include/mewzoom_hip.h states them next to
mz_image_view), one table run against all six entries -- mz_forward_view, mz_metrics, mz_resize, mz_blur, mz_noise, mz_jpeg -- on a
machine without a device: each case is MZ_ERR_INVALID_ARGUMENT with a message, and what the view checks accept reaches the entry's next
check.  The per-entry files (test_views_cpu.py, test_metrics_cpu.py, test_resize_cpu.py, test_degrade_cpu.py) hold each entry's own
refusals."""

from ctypes import byref, c_void_p

import pytest

from golden_util import GoldenCase
from ultrazoom_amd import _ffi

H, W = 48, 64          # the input of every entry
FAKE, FAKE2 = 0x10000, 0x40000000  # never dereferenced: validation comes first; far enough apart for any B used here
MISSING_WEIGHTS = -4


def dense(h, w):
    return (3 * h * w, h * w, w, 1)


# entry -> (output side lengths, one past the element range, B is bounded by 65535, the second view is written)
ENTRIES = {
    "forward_view": ((2 * H, 2 * W), 2, False, True),  # g1_2x_c16: the output is 96 x 128
    "metrics": ((H, W), 4, True, False),               # the second view is `target`: read, so its strides may be 0
    "resize": ((24, 40), 4, True, True),
    "blur": ((H, W), 4, True, True),
    "noise": ((H, W), 4, True, True),
    "jpeg": ((H, W), 4, True, True),
}


@pytest.fixture(scope="module")
def handle():
    h = _ffi.Handle(GoldenCase("g1_2x_c16").config, _ffi.MZ_F32)  # holds no weights: mz_forward_view stops there at the latest
    yield h
    h.close()


def call(entry, handle, x="dense", out="dense", elem=0, batch=2):
    """The entry on otherwise valid arguments, its workspace 8 bytes short (mz_blur and mz_noise, which have none: a negative sigma), so
    that a call the view checks accept stops at the entry's next check without a device."""
    (ho, wo), _, _, _ = ENTRIES[entry]
    x = _ffi.view(FAKE, dense(H, W)) if x == "dense" else x
    out = _ffi.view(FAKE2, dense(ho, wo)) if out == "dense" else out
    xp, op = (byref(x) if x is not None else None), (byref(out) if out is not None else None)
    lib, ws = _ffi.lib(), c_void_p(FAKE)
    if entry == "forward_view":
        code = lib.mz_forward_view(handle.ptr, xp, op, None, batch, H, W, 1, elem, None, ws, 1 << 40, 0, None)
    elif entry == "metrics":
        code = lib.mz_metrics(xp, op, elem, batch, H, W, 1, -1.0, 2.0, ws, ws, 8, None)
    elif entry == "resize":
        code = lib.mz_resize(xp, op, elem, batch, H, W, ho, wo, 0, 0, None, ws, 8, None)
    elif entry == "blur":
        code = lib.mz_blur(xp, op, elem, batch, H, W, -1.0, None)
    elif entry == "noise":
        code = lib.mz_noise(xp, op, elem, batch, H, W, -1.0, 1, 0, None)
    else:
        code = lib.mz_jpeg(xp, op, elem, batch, H, W, 50, ws, 8, None)
    return code, lib.mz_last_error().decode()


def refused(entry):
    (ho, wo), elem_end, bounded, writes = ENTRIES[entry]
    d = dense(ho, wo)
    cases = {
        "null input view": dict(x=None),
        "null output view": dict(out=None),
        "null input data": dict(x=_ffi.view(None, dense(H, W))),
        "null output data": dict(out=_ffi.view(None, d)),
        "elem -1": dict(elem=-1),
        f"elem {elem_end}": dict(elem=elem_end),
        "no images": dict(batch=0),
    }
    if bounded:
        cases["65536 images"] = dict(batch=65536)
    if writes:
        cases["output channel stride 0"] = dict(out=_ffi.view(FAKE2, (d[0], 0, d[2], 1)))
        cases["output row stride 0"] = dict(out=_ffi.view(FAKE2, (d[0], d[1], 0, 1)))
        cases["output column stride 0"] = dict(out=_ffi.view(FAKE2, (d[0], d[1], d[2], 0)))
        cases["output image stride 0 with two images"] = dict(out=_ffi.view(FAKE2, (0,) + d[1:]))
    return cases


def accepted(entry):
    (ho, wo), _, _, writes = ENTRIES[entry]
    d, di = dense(ho, wo), dense(H, W)
    cases = {
        "dense": dict(),
        "negative strides (BGR, bottom-up)": dict(x=_ffi.view(FAKE + 4 * (3 * H * W - 1), (di[0], -di[1], -di[2], 1)),
                                                  out=_ffi.view(FAKE2 + 4 * 2 * d[1], (d[0], -d[1], d[2], 1))),
        "input strides of 0": dict(x=_ffi.view(FAKE, (0, 0, 0, 0))),
        "output image stride 0 with one image": dict(out=_ffi.view(FAKE2, (0,) + d[1:]), batch=1),
    }
    if not writes:
        cases["second view with strides of 0"] = dict(out=_ffi.view(FAKE2, (0, 0, 0, 0)))
    return cases


REFUSED = [(e, n, a) for e in ENTRIES for n, a in refused(e).items()]
ACCEPTED = [(e, n, a) for e in ENTRIES for n, a in accepted(e).items()]


@pytest.mark.parametrize("entry, name, args", REFUSED, ids=[f"{e}: {n}" for e, n, _ in REFUSED])
def test_shared_refusals(handle, entry, name, args):
    code, msg = call(entry, handle, **args)
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (entry, name, code, msg)
    assert msg, (entry, name)


@pytest.mark.parametrize("entry, name, args", ACCEPTED, ids=[f"{e}: {n}" for e, n, _ in ACCEPTED])
def test_what_the_view_checks_accept_reaches_the_next_check(handle, entry, name, args):
    code, msg = call(entry, handle, **args)
    if entry == "forward_view":
        assert code == MISSING_WEIGHTS and "has not been set" in msg, (name, code, msg)
    elif entry in ("blur", "noise"):
        assert code == _ffi.MZ_ERR_INVALID_ARGUMENT and msg.startswith("sigma -1"), (name, code, msg)
    else:
        assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL and "workspace too small" in msg, (name, code, msg)


def test_the_checks_survive_extreme_values_under_the_sanitizers(tmp_path):
    """tests/view_check_main.cpp -- strides of INT64_MAX / INT64_MIN / -1, sides of 2^28, 65535 images, windows at INT32_MAX, addresses
    at the top of the address space, and the ordinary overlap cases -- built from the host check header alone with the address and
    undefined-behaviour sanitizers: a signed overflow in a check ends it.  A stand-alone host program: nothing of it is loaded here."""
    import shutil
    import subprocess
    from pathlib import Path

    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = Path(__file__).resolve().parent / "view_check_main.cpp"
    exe = tmp_path / "view_check_main"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "view checks OK" in run.stdout and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
