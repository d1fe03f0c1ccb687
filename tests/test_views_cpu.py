"""mz_forward_view refuses bad views, windows and element codes before it looks at the weights or touches a GPU: every case runs on
a handle that holds no weights, on a machine without a device."""

from ctypes import byref, c_int32, c_int64, c_void_p

import pytest

from golden_util import GoldenCase
from ultrazoom_amd import _ffi

B, H, W, R = 2, 37, 45, 2  # g1_2x_c16: the output is 74 x 90
DENSE_IN = (3 * H * W, H * W, W, 1)
DENSE_OUT = (3 * R * H * R * W, R * H * R * W, R * W, 1)
FAKE = 0x10000  # never dereferenced: validation comes first


def view(data=FAKE, strides=DENSE_IN):
    return _ffi.MzImageView(c_void_p(data), (c_int64 * 4)(*strides))


def call(handle, x, out, elem=0, window=None, batch=B):
    win = (c_int32 * 4)(*window) if window is not None else None
    code = _ffi.lib().mz_forward_view(
        handle.ptr, byref(x) if x is not None else None, byref(out) if out is not None else None, None, batch, H, W, 1, elem, win,
        c_void_p(FAKE), 1 << 40, 0, None,
    )
    return code, _ffi.lib().mz_last_error().decode()


@pytest.fixture(scope="module")
def handle():
    h = _ffi.Handle(GoldenCase("g1_2x_c16").config, _ffi.MZ_F32)
    yield h
    h.close()


REFUSED = {
    "null input view": dict(x=None),
    "null output view": dict(out=None),
    "null input data": dict(x=view(data=None)),
    "null output data": dict(out=view(data=None, strides=DENSE_OUT)),
    "elem 2": dict(elem=2),
    "elem -1": dict(elem=-1),
    "window without rows": dict(window=(0, 0, 0, 10)),
    "window without columns": dict(window=(0, 0, 10, 0)),
    "window of negative height": dict(window=(4, 4, -2, 10)),
    "window above the output": dict(window=(-1, 0, 10, 10)),
    "window left of the output": dict(window=(0, -1, 10, 10)),
    "window past the last row": dict(window=(R * H - 1, 0, 2, 10)),
    "window past the last column": dict(window=(0, R * W - 1, 10, 2)),
    "window origin outside": dict(window=(R * H, R * W, 1, 1)),
    "output channel stride 0": dict(out=view(strides=(DENSE_OUT[0], 0, DENSE_OUT[2], 1))),
    "output row stride 0": dict(out=view(strides=(DENSE_OUT[0], DENSE_OUT[1], 0, 1))),
    "output column stride 0": dict(out=view(strides=(DENSE_OUT[0], DENSE_OUT[1], DENSE_OUT[2], 0))),
    "output image stride 0, two images": dict(out=view(strides=(0,) + DENSE_OUT[1:])),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_bad_arguments_are_refused_before_weights_and_gpu(handle, name):
    args = dict(x=view(), out=view(strides=DENSE_OUT))
    args.update(REFUSED[name])
    code, msg = call(handle, **args)
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (name, code, msg)
    assert msg, name


def test_valid_views_reach_the_weights_check(handle):
    """What validation lets through stops at the next check, the missing weights -- still without a GPU call: the whole output and its
    last pixel as windows, signed strides (BGR), input strides of 0, an output image stride of 0 for a single image."""
    bgr_in = (3 * H * W, -H * W, W, 1)
    for args in (
        dict(),
        dict(elem=1),
        dict(window=(0, 0, R * H, R * W)),
        dict(window=(R * H - 1, R * W - 1, 1, 1)),
        dict(x=view(strides=bgr_in), out=view(strides=(DENSE_OUT[0], -DENSE_OUT[1], DENSE_OUT[2], 1))),
        dict(x=view(strides=(0, 0, 0, 0))),
        dict(out=view(strides=(0,) + DENSE_OUT[1:]), batch=1),
    ):
        full = dict(x=view(), out=view(strides=DENSE_OUT))
        full.update(args)
        code, msg = call(handle, **full)
        assert code == -4 and "has not been set" in msg, (args, code, msg)  # MZ_ERR_MISSING_WEIGHTS


def test_null_handle_is_refused():
    code = _ffi.lib().mz_forward_view(None, byref(view()), byref(view(strides=DENSE_OUT)), None, B, H, W, 1, 0, None, c_void_p(FAKE), 1 << 40,
                                      0, None)
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT
