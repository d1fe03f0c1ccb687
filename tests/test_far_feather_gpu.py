"""mz_feather_paste on far views (tests/far_util.py), in the manner of tests/test_far_views_gpu.py: src and dst each inside one large
allocation at strides whose offsets cross 2^31 and 2^32 -- an image stride of 2^31 + 40 elements, a channel stride past 2^32 bytes, a
row pitch of 2^28 + 64 bytes, the last also bottom-up.  misalign = 0 keeps the base and every stride a multiple of 16 bytes, so the
16-byte path runs at the far offsets; an odd number of elements breaks rows_aligned and the element path runs there.  The result has
the bits of the reference, src is unchanged, and the 64-byte guard bands around every row of both views are intact.

Sizes.  The image is (2, 3, 18, 40) with ramps (6, 10).  Two far views live at once and together stay under far_util.MAX_DEVICE_BYTES:
the image kind in uint8, bf16 and f32 (2^31 elements a view: 2.1, 4.3 and 8.6 GB), the pitch kinds in every type (35 pitches: 9.4 GB a
view whatever the element).  A channel stride of 2^32 bytes puts the second image of ONE view past the cap (5 strides: 21.5 GB), so
the channel kind runs one image, (1, 3, 18, 40): 8.6 GB a view."""

import gc

import pytest
import torch

import far_util as fu
import feather_ref
from feather_ref import DTYPES, ELEM, same_bits
from ultrazoom_amd import _ffi

pytestmark = pytest.mark.gpu

H, W, RAMP = 18, 40, (6, 10)
KINDS = ("image", "channel", "pitch", "pitch_neg")


@pytest.fixture(autouse=True)
def release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_paste_on_far_views(kind, misalign):
    B = 1 if kind == "channel" else 2
    for dt in ("u8", "bf16", "f32"):
        src, dst = feather_ref.pair(B, H, W, dt, RAMP)
        want = feather_ref.expected(B, H, W, dt, RAMP)
        es = src.element_size()
        assert 2 * fu.far_layout(src.shape, es, kind, misalign).nbytes < fu.MAX_DEVICE_BYTES
        s = fu.far_view(src, kind, misalign, device="cuda")
        d = fu.far_view(dst, kind, misalign, device="cuda")
        vec = all(v.ptr % 16 == 0 and all(st * es % 16 == 0 for st in v.strides[:3]) for v in (s, d))
        assert vec == (misalign == 0)
        _ffi.feather_paste(s.pair, d.pair, ELEM[dt], B, H, W, RAMP[0], RAMP[1], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        s.check_guards()
        d.check_guards()
        assert same_bits(d.read(), want), (kind, misalign, dt)
        assert torch.equal(feather_ref.bits(s.read().cpu()), feather_ref.bits(src)), "the paste changed src"
        del s, d
        gc.collect()
        torch.cuda.empty_cache()
