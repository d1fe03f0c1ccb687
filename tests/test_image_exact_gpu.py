"""mz_interpolate (bilinear, bicubic), mz_resize and mz_blur bit for bit against the arithmetic their headers state, restated in
tests/image_exact.py: float64 fma sums in ascending tap order, the stated intermediate, the stated roundings.  Every assertion is an
equality of bit patterns (NaN compares as NaN) over ALL elements of a result.  The cases (image_exact.CASES) are the smallest shapes that
reach each path of the kernels, in all four element types; besides uniform noise their inputs put inputs and results into the subnormals
of the stored type (with -0 among the results), past the float16 maximum, onto rounding ties of the stored type and one input unit
beside them, onto an infinity and a NaN, and onto sums that cancel down to the rounding of one input, where a product rounded before it
is added or another order of the taps shows in the float32 result.  tests/test_image_exact_cpu.py shows what these cases tell apart."""

import pytest
import torch

import degrade_ref
import image_exact as ie
from interp_util import hip_interp
from resize_util import hip_resize

pytestmark = pytest.mark.gpu


def run(c: ie.Case, x: torch.Tensor, monkeypatch) -> torch.Tensor:
    if c.op == "blur":
        return degrade_ref.hip().gaussian_blur(x, c.how)
    size, window = c.shape[1], ie.window_of(c)
    if c.op == "resize":
        return hip_resize(x, size, filter=c.how, clamp=bool(c.clamp), window=window)
    if c.via == "gather":
        monkeypatch.setenv("MZ_INTERP_GATHER", "1")
        got = hip_interp(x, size, mode=c.how, clamp=bool(c.clamp))
        torch.cuda.synchronize()
        monkeypatch.delenv("MZ_INTERP_GATHER")
        return got
    if c.via == "strided":  # every second column of a canvas: stored element by element
        canvas = torch.zeros((x.shape[0], 3, size[0], 2 * size[1]), dtype=x.dtype, device="cuda")
        got = hip_interp(x, size, mode=c.how, clamp=bool(c.clamp), out=canvas[..., ::2])
        assert got.stride(3) == 2 and not bool(canvas[..., 1::2].any())
        return got
    return hip_interp(x, size, mode=c.how, clamp=bool(c.clamp), window=window)


@pytest.mark.parametrize("p", ie.PAIRS, ids=ie.pair_id)
def test_the_device_gives_the_bits_of_the_stated_arithmetic(p, monkeypatch):
    c, dt = p
    monkeypatch.delenv("MZ_INTERP_GATHER", raising=False)
    want = ie.case_expected(c, dt).want
    if c.kind == "ties":
        even, odd, beside = ie.tie_census(c, dt, ie.case_input(c, dt))
        assert min(even, odd, beside) >= ie.MIN_TIES, (even, odd, beside)
    got = run(c, ie.case_input(c, dt).cuda(), monkeypatch).cpu()
    same = ie.same_bits(got, want)
    wrong = (~same).nonzero()
    print(f"{ie.pair_id(p)}: {len(wrong)} of {same.numel()} elements differ")
    assert len(wrong) == 0, [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in wrong[:8]]
