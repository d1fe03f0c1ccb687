"""mz_metrics / mz_metrics_workspace_bytes without a GPU: the declarations, the workspace sizes, every refused argument (refused before
anything touches a device), and the Python layer's refusals."""

import re
from ctypes import byref, c_int64, c_size_t, c_void_p
from pathlib import Path

import pytest
import torch

from ultrazoom_amd import _ffi
from ultrazoom_amd.evaluate import evaluate
from ultrazoom_amd.synth import synth_image

REPO = Path(__file__).resolve().parent.parent
B, H, W = 2, 48, 64
DENSE = (3 * H * W, H * W, W, 1)
FAKE = 0x10000  # never dereferenced: validation comes first
ALL = 7


def view(data=FAKE, strides=DENSE):
    return _ffi.MzImageView(c_void_p(data), (c_int64 * 4)(*strides))


def call(pred=view(), target=view(), elem=0, batch=B, h=H, w=W, which=ALL, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
    code = _ffi.lib().mz_metrics(
        byref(pred) if pred is not None else None, byref(target) if target is not None else None, elem, batch, h, w, which, -1.0, 2.0,
        c_void_p(out) if out else None, c_void_p(ws) if ws else None, ws_bytes, None,
    )
    return code, _ffi.lib().mz_last_error().decode()


def workspace(batch, h, w, which):
    n = c_size_t()
    code = _ffi.lib().mz_metrics_workspace_bytes(batch, h, w, which, byref(n))
    return code, int(n.value)


def test_header_declares_and_library_exports_both_entries():
    text = (REPO / "include" / "mewzoom_hip.h").read_text()
    assert re.search(r"\bint mz_metrics_workspace_bytes\(int B, int H, int W, int which, size_t\* bytes\);", text)
    assert re.search(r"\bint mz_metrics\(const mz_image_view\* pred, const mz_image_view\* target, int elem,", text)
    m = re.search(r"#define MZ_METRIC_SLOTS (\d+)", text)
    assert m and int(m.group(1)) == _ffi.MZ_METRIC_SLOTS
    lib = _ffi.lib()
    assert lib.mz_metrics and lib.mz_metrics_workspace_bytes


def test_workspace_grows_with_the_batch_and_is_small_for_psnr_alone():
    for which in (1, 2, 4, 3, 7):
        sizes = [workspace(b, H, W, which) for b in (1, 2, 3, 8)]
        assert all(code == 0 for code, _ in sizes), sizes
        assert all(a[1] <= b[1] for a, b in zip(sizes, sizes[1:])), (which, sizes)
        assert sizes[0][1] < sizes[-1][1], (which, sizes)
    # PSNR alone: a few partial sums per image, however large the images are (here one pair of 4320 x 7680 images: 796 MB of bf16)
    code, n = workspace(1, 4320, 7680, 1)
    assert code == 0 and n <= 64 * 1024, n
    # VIF keeps its float64 pyramid there: about (1/4 + 1/16 + 1/64) x 2 images x 8 bytes per pixel
    code, n = workspace(1, 1080, 1920, 4)
    assert code == 0 and 3 * 1080 * 1920 * 16 * 0.30 < n < 3 * 1080 * 1920 * 16 * 0.36, n


REFUSED = {
    "null pred view": dict(pred=None),
    "null target view": dict(target=None),
    "null pred data": dict(pred=view(data=None)),
    "null target data": dict(target=view(data=None)),
    "elem -1": dict(elem=-1),
    "elem 4": dict(elem=4),
    "which 0": dict(which=0),
    "which 8": dict(which=8),
    "which -1": dict(which=-1),
    "which with an unknown bit": dict(which=9),
    "no images": dict(batch=0),
    "no rows": dict(h=0, which=1),
    "no columns": dict(w=0, which=1),
    "negative width": dict(w=-3, which=1),
    "10 rows with SSIM": dict(h=10, which=2),
    "10 columns with SSIM": dict(w=10, which=3),
    "40 rows with VIF": dict(h=40, which=4),
    "40 columns with VIF": dict(w=40, which=7),
    "null out_dev": dict(out=None),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_bad_arguments_are_refused_before_the_gpu(name):
    code, msg = call(**REFUSED[name])
    assert code == _ffi.MZ_ERR_INVALID_ARGUMENT, (name, code, msg)
    assert msg, name


def test_small_images_pass_for_the_metrics_that_fit_and_a_short_workspace_is_refused():
    """What validation lets through stops at the next check, the workspace -- still without a GPU call: 1 x 1 for PSNR, 11 x 11 for
    SSIM, 41 x 41 for VIF, every element type, signed strides and strides of 0."""
    for args in (
        dict(h=1, w=1, which=1), dict(h=11, w=11, which=3), dict(h=41, w=41, which=7), dict(elem=1), dict(elem=2), dict(elem=3),
        dict(pred=view(strides=(DENSE[0], -DENSE[1], DENSE[2], 1))), dict(target=view(strides=(0, 0, 0, 0))),
    ):
        code, msg = call(ws_bytes=8, **args)
        assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL and "workspace too small" in msg, (args, code, msg)
    code, msg = call(ws=None)
    assert code == _ffi.MZ_ERR_WORKSPACE_TOO_SMALL, (code, msg)
    for bad in (dict(batch=0, h=H, w=W, which=7), dict(batch=1, h=10, w=W, which=2), dict(batch=1, h=H, w=40, which=4),
                dict(batch=1, h=H, w=W, which=0), dict(batch=1, h=H, w=W, which=16)):
        assert workspace(**bad)[0] == _ffi.MZ_ERR_INVALID_ARGUMENT, bad
    assert _ffi.lib().mz_metrics_workspace_bytes(1, H, W, 7, None) == _ffi.MZ_ERR_INVALID_ARGUMENT


def test_image_metrics_refuses_cpu_tensors():
    from ultrazoom_amd.metrics import image_metrics

    x = synth_image(1, 48, 48, seed=1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        image_metrics(x, x)
    with pytest.raises(ValueError, match="which"):
        image_metrics(x, x, which=("lpips",))


def test_evaluate_default_backend_is_unchanged():
    class Nearest:
        def upscale(self, x):
            return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")

    hr = synth_image(3, 48, 44, seed=5)
    lr = hr[:, :, ::2, ::2]
    pairs = [(lr[:2], hr[:2]), (lr[2:], hr[2:])]
    assert evaluate(Nearest(), pairs, backend="torch") == evaluate(Nearest(), pairs)
    assert evaluate(Nearest(), pairs)["vif"] is not None
    with pytest.raises(ValueError, match="backend"):
        evaluate(Nearest(), pairs, backend="numpy")
    with pytest.raises(RuntimeError, match="MI355X only"):
        evaluate(Nearest(), pairs, backend="hip")
