"""tests/poison_util.py on the CPU: a clean round passes; one byte written into each kind of guard, or into an input, is reported
with the tensor's name, the side and the byte offset."""

import re

import pytest
import torch

from poison_util import ALIGN, MIN_GUARD, Arena, pattern


def build():
    a = Arena("cpu", capacity=4 << 20)
    x = a.input(torch.arange(5 * 77, dtype=torch.float32).reshape(5, 77), name="x")
    img = a.input(torch.arange(3 * 100, dtype=torch.uint8).reshape(3, 100), name="img", fill=0x00)
    out = a.output((3, 2, 50), torch.bfloat16, name="out")
    ws = a.raw(100_000, 0xFF, name="ws")
    return a, x, img, out, ws


def region(a, name):
    return next(r for r in a.regions if r["name"] == name)


def test_layout_alignment_guard_sizes_and_fills():
    a, x, img, out, ws = build()
    assert torch.equal(x, torch.arange(5 * 77, dtype=torch.float32).reshape(5, 77)) and x.is_contiguous()
    assert out.shape == (3, 2, 50) and out.dtype == torch.bfloat16 and bool((out == 7.0).all())
    assert ws.dtype == torch.uint8 and ws.numel() == 100_000 and bool((ws == 0xFF).all())
    prev_back = 0
    for r, t in zip(a.regions, (x, img, out, ws)):
        nbytes = t.numel() * t.element_size()
        assert r["end"] - r["start"] == nbytes
        assert t.data_ptr() == a.buf.data_ptr() + r["start"] and t.data_ptr() % ALIGN == 0
        assert r["front"] == prev_back, "regions must not overlap"
        for lo, hi in ((r["front"], r["start"]), (r["end"], r["back"])):
            assert hi - lo >= max(nbytes, MIN_GUARD)
        prev_back = r["back"]
    assert prev_back <= a.buf.numel()
    # input guards: the fill byte (0xFF is NaN in every float type); output and workspace guards: the position-dependent pattern
    rx, ri, ro = region(a, "x"), region(a, "img"), region(a, "out")
    assert bool((a.buf[rx["front"] : rx["start"]] == 0xFF).all()) and bool((a.buf[rx["end"] : rx["back"]] == 0xFF).all())
    assert bool((a.buf[ri["front"] : ri["start"]] == 0).all()) and bool((a.buf[ri["end"] : ri["back"]] == 0).all())
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert bool(torch.isnan(a.buf[rx["front"] : rx["start"]].view(dt)).all())
    g = a.buf[ro["end"] : ro["back"]]
    assert g[0].item() == (131 * ro["end"] + 17) & 255 and g[5].item() == (131 * (ro["end"] + 5) + 17) & 255
    assert len(set(g[:256].tolist())) == 256, "every byte value appears: no constant store can match the pattern"


def test_a_clean_round_passes():
    a, x, img, out, ws = build()
    out.copy_(torch.randn(3, 2, 50).to(torch.bfloat16))  # outputs and workspaces are the call's to write, wholly
    ws.fill_(3)
    a.check()
    a.check()


GUARD_HITS = [
    # tensor, kind, side, offset inside that side (-1: its last byte)
    ("out", "output", "front guard", -1),
    ("out", "output", "back guard", 0),
    ("out", "output", "back guard", 4097),
    ("ws", "raw", "front guard", 12345),
    ("ws", "raw", "back guard", -1),
    ("x", "input", "front guard", -1),
    ("x", "input", "back guard", 0),
    ("x", "input", "contents", 4 * 77 + 2),
    ("img", "input", "contents", 299),
    ("img", "input", "back guard", 60000),
]


@pytest.mark.parametrize("name,kind,side,off", GUARD_HITS)
def test_one_byte_is_reported_with_name_side_and_offset(name, kind, side, off):
    a, *_ = build()
    r = region(a, name)
    lo, hi = {"front guard": (r["front"], r["start"]), "contents": (r["start"], r["end"]), "back guard": (r["end"], r["back"])}[side]
    if off < 0:
        off += hi - lo
    a.buf[lo + off] ^= 0x40
    with pytest.raises(AssertionError) as e:
        a.check()
    msg = str(e.value)
    assert f"{kind} '{name}'" in msg and side in msg, msg
    assert int(re.search(r"byte offset (\d+)", msg).group(1)) == off, msg


def test_the_first_of_several_bytes_is_the_one_reported_and_a_store_of_zeros_shows():
    a, *_ = build()
    r = region(a, "out")
    want = pattern(r["end"], r["back"], "cpu")
    zero_at = int(torch.nonzero(want == 0)[0, 0])  # the one byte in 256 where a stray zero equals the pattern
    a.buf[r["end"] + zero_at : r["end"] + zero_at + 16] = 0  # a 16-byte store of zeros, as a stray plane entry would be
    with pytest.raises(AssertionError, match=rf"output 'out': back guard changed at byte offset {zero_at + 1} "):
        a.check()


def test_a_full_arena_and_a_repeated_name_are_refused():
    a = Arena("cpu", capacity=3 * MIN_GUARD)
    a.raw(1000, 0, name="w")
    with pytest.raises(MemoryError):
        a.raw(1000, 0, name="v")
    b = Arena("cpu", capacity=1 << 20)
    b.raw(16, 0, name="w")
    with pytest.raises(ValueError):
        b.raw(16, 0, name="w")
