"""Poisoned surroundings for the kernels' tensors: nothing outside a tensor may be read, nothing outside an output written.

An Arena is ONE uint8 allocation.  Every tensor carved from it (at a 256-byte aligned offset) has a guard band in front and one
behind, each at least as large as the tensor and at least 64 KiB: a slip of a whole row, plane or image still lands in a guard --
in memory the test owns, where it becomes a failed assertion and never a fault.

  input(t)        guards of 0xFF bytes (NaN as f32, bf16 and f16; uint8 callers also run with fill=0x00): a read outside the tensor
                  poisons the result.  check() compares the tensor AND its guards with what was put in: kernels do not write inputs.
  output(shape)   guards of a position-dependent byte pattern, so that a stray store of zeros, of NaN or of data shows alike.
  raw(nbytes)     a workspace pre-filled with one byte value, pattern guards.
  check()         after the call and a synchronise; an AssertionError names the tensor, the side and the first offending byte.
"""

from __future__ import annotations

import torch

ALIGN = 256
MIN_GUARD = 64 * 1024


def pattern(start: int, end: int, device) -> torch.Tensor:
    """The guard pattern of arena bytes [start, end): (131 * i + 17) & 255 at arena offset i."""
    i = torch.arange(start, end, dtype=torch.int64, device=device) & 255  # (131 is odd: the pattern has period 256)
    return ((i * 131 + 17) & 255).to(torch.uint8)


def _up(v: int) -> int:
    return (v + ALIGN - 1) // ALIGN * ALIGN


def room(*nbytes: int) -> int:
    """The capacity an Arena needs for tensors of these sizes."""
    return sum(_up(n) + 2 * _up(max(n, MIN_GUARD)) for n in nbytes)


class Arena:
    def __init__(self, device, capacity: int = 64 << 20):
        self.device = torch.device(device)
        whole = torch.empty(capacity + ALIGN, dtype=torch.uint8, device=self.device)
        skip = -whole.data_ptr() % ALIGN  # (a CPU allocation is aligned to 64 bytes only)
        self.buf = whole[skip : skip + capacity]
        self.used = 0
        self.regions = []  # dicts: name, kind, front, start, end, back (arena byte offsets: guards are [front, start) and [end, back))
        self.kept = {}     # inputs: name -> a copy of arena bytes [front, back)

    def _carve(self, name, kind: str, nbytes: int) -> dict:
        guard = _up(max(nbytes, MIN_GUARD))
        front = self.used
        start = front + guard                 # used and guard are multiples of ALIGN, and so is the tensor's offset
        end = start + nbytes
        back = _up(end) + guard
        if back > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is full: {name!r} needs bytes up to {back}")
        if (self.buf.data_ptr() + start) % ALIGN:
            raise RuntimeError("the arena's own allocation is not 256-byte aligned")
        r = dict(name=name or f"{kind}{len(self.regions)}", kind=kind, front=front, start=start, end=end, back=back)
        if any(o["name"] == r["name"] for o in self.regions):
            raise ValueError(f"two tensors named {r['name']!r}")
        self.regions.append(r)
        self.used = back
        return r

    def _view(self, r: dict, shape, dtype) -> torch.Tensor:
        return self.buf[r["start"] : r["end"]].view(dtype).view(shape)

    def input(self, t: torch.Tensor, name: str = None, fill: int = 0xFF) -> torch.Tensor:
        """A copy of `t` (already in the library's layout and dtype) between guards of `fill` bytes."""
        t = t.contiguous()
        r = self._carve(name, "input", t.numel() * t.element_size())
        self.buf[r["front"] : r["back"]] = fill
        v = self._view(r, t.shape, t.dtype)
        v.copy_(t)
        self.kept[r["name"]] = self.buf[r["front"] : r["back"]].clone()
        return v

    def _pattern_guards(self, r: dict) -> None:
        self.buf[r["front"] : r["start"]] = pattern(r["front"], r["start"], self.device)
        self.buf[r["end"] : r["back"]] = pattern(r["end"], r["back"], self.device)

    def output(self, shape, dtype, fill=7.0, name: str = None) -> torch.Tensor:
        """An output tensor pre-filled with `fill`, between pattern guards."""
        n = 1
        for s in shape:
            n *= s
        r = self._carve(name, "output", n * torch.empty((), dtype=dtype).element_size())
        self._pattern_guards(r)
        v = self._view(r, tuple(shape), dtype)
        v.fill_(fill)
        return v

    def raw(self, nbytes: int, fill: int, name: str = None) -> torch.Tensor:
        """A workspace of `nbytes` bytes, every byte `fill`, between pattern guards."""
        r = self._carve(name, "raw", nbytes)
        self._pattern_guards(r)
        v = self.buf[r["start"] : r["end"]]
        v.fill_(fill)
        return v

    @staticmethod
    def _first_difference(got: torch.Tensor, want: torch.Tensor):
        if torch.equal(got, want):
            return None
        return int(torch.nonzero(got != want)[0, 0])

    def _fail(self, r: dict, side: str, off: int, got: int, want: int):
        raise AssertionError(f"{r['kind']} {r['name']!r}: {side} changed at byte offset {off} of it (0x{got:02x}, was 0x{want:02x})")

    def check(self) -> None:
        """Every guard still holds what it held, and every input is byte for byte what was put in."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for r in self.regions:
            sides = (("front guard", r["front"], r["start"]), ("contents", r["start"], r["end"]), ("back guard", r["end"], r["back"]))
            for side, a, b in sides:
                if r["kind"] == "input":
                    want = self.kept[r["name"]][a - r["front"] : b - r["front"]]
                elif side == "contents":
                    continue  # outputs and workspaces are the call's to write
                else:
                    want = pattern(a, b, self.device)
                got = self.buf[a:b]
                off = self._first_difference(got, want)
                if off is not None:
                    self._fail(r, side, off, int(got[off]), int(want[off]))
