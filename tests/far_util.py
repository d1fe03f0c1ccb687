"""Far views and long walks of the image entries (tests/test_far_views_cpu.py, tests/test_far_views_gpu.py, tests/test_long_walk_gpu.py).
Needs no GPU: every function takes a device, and the CPU tests run all of them at small sizes before they judge a kernel.

  far_layout, far_view   a dense [B, C, H, W] tensor inside ONE large torch.empty allocation, at strides whose byte and element offsets
                         cross 2^31 and 2^32; only the view's elements and the 64-byte guard bands around its rows are ever written
  hashed_codes, code_of  integer codes from a multiplicative hash of the global row index g = b H + row, built chunk by chunk
  lut_check              out == lut[codes] over a whole plane, chunk by chunk, on the device the planes live on
  WALKS, walk_blocks     the sizes of the long-walk cases and the small blocks that are copied to the host
  noise_blocks, noise_expected
                         the blocks of the tall noise frame and their bytes from degrade_ref's Philox and Box-Muller

The kinds of far_view.  `big` replaces the large stride (the CPU tests: the same code at strides of a few kilobytes):
  image      image stride 2^31 + 40 elements (uint8: + 48, the next multiple of 16 bytes); rows 128 bytes apart from each other's ends
  image_neg  the same, negative: the pointer names image B - 1
  channel    channel stride 2^32 + 64 BYTES: channel 1 starts past 2^32 bytes, and in the 16-bit types its element offset past 2^31 and
             channel 2's past 2^32
  pitch      row pitch 2^28 + 64 bytes, the channels of a row side by side inside the pitch: rows >= 8 start past 2^31 bytes, rows >= 16
             past 2^32
  pitch_neg  the same, bottom-up: the pointer names row H - 1
misalign (an odd number of elements) is added to the base and to the large stride: rows_aligned (mz_view.h) is then false and the
element paths run; with misalign = 0 the base and every stride are multiples of 16 bytes and the 16-byte paths run at the far offsets."""

from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import degrade_ref
from poison_util import pattern

MAX_DEVICE_BYTES = 20e9  # the cap of tests/test_large_offsets_gpu.py
GUARD = 64               # bytes in front of and behind every row of a far view
FRONT = 256              # bytes of the allocation in front of the view's lowest element (room for the first guard; a multiple of 16)
KINDS = ("image", "image_neg", "channel", "pitch", "pitch_neg")
PITCH_H = 18

Layout = namedtuple("Layout", "kind shape es tbase tstrides kbase kstrides nbytes")
# tbase (bytes), tstrides (elements, all positive): the view as torch addresses it; kbase, kstrides: element (0, 0, 0, 0) and the signed
# strides as the KERNEL is told (a negative kind: image b of the kernel is image B - 1 - b of the torch view, row y is row H - 1 - y)


def _up16(n: int) -> int:
    return (n + 15) // 16 * 16


def big_stride_bytes(kind: str, es: int) -> int:
    """the large stride of a kind, in bytes, at misalign = 0"""
    if kind.startswith("image"):
        return _up16(((1 << 31) + 40) * es)
    return (1 << 32) + 64 if kind == "channel" else (1 << 28) + 64


def far_layout(shape, es: int, kind: str, misalign: int = 0, big: int | None = None) -> Layout:
    """Where the elements of a [B, C, H, W] view of `es`-byte elements lie; allocates nothing.  big: the large stride in bytes."""
    B, C, H, W = (int(v) for v in shape)
    assert kind in KINDS and es in (1, 2, 4) and (misalign == 0 or misalign % 2 == 1)
    big = big_stride_bytes(kind, es) if big is None else big
    assert big % 16 == 0
    rowb = _up16(W * es) + 2 * GUARD  # from one row's first byte to the next's: the row, its back guard, the next one's front guard
    large = big // es + misalign
    if kind.startswith("image"):
        rs, cs, s0 = rowb // es, H * rowb // es, large
        assert s0 >= C * cs, "the images would overlap"
    elif kind == "channel":
        rs, cs = rowb // es, large
        assert cs >= H * rs, "the channels would overlap"
        s0 = C * cs
    else:
        cs, rs = rowb // es, large
        assert rs >= C * cs, "the rows would overlap"
        s0 = H * rs
    tbase = FRONT + misalign * es
    span = (B - 1) * s0 + (C - 1) * cs + (H - 1) * rs
    nbytes = tbase + span * es + rowb + FRONT
    kbase, ks = tbase, [s0, cs, rs, 1]
    if kind == "image_neg":
        kbase, ks[0] = tbase + (B - 1) * s0 * es, -s0
    if kind == "pitch_neg":
        kbase, ks[2] = tbase + (H - 1) * rs * es, -rs
    return Layout(kind, (B, C, H, W), es, tbase, (s0, cs, rs, 1), kbase, tuple(ks), nbytes)


def element_offsets(L: Layout):
    """byte offset from the kernel's pointer of the first element of every (image, channel, row): numpy int64 [B, C, H]"""
    B, C, H, _ = L.shape
    b, c, y = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(C, dtype=np.int64), np.arange(H, dtype=np.int64), indexing="ij")
    return (b * L.kstrides[0] + c * L.kstrides[1] + y * L.kstrides[2]) * L.es


class FarView:
    """One far view: `alloc` (uint8, the whole allocation), `pair` = (address of element (0, 0, 0, 0), signed element strides) for
    _ffi.view, write(dense) / read() in the KERNEL's order of images and rows, fill_guards() / check_guards()."""

    def __init__(self, L: Layout, dtype, device):
        assert L.nbytes < MAX_DEVICE_BYTES, f"a far view of {L.nbytes / 1e9:.2f} GB"
        self.layout, self.dtype = L, dtype
        self.alloc = torch.empty(L.nbytes, dtype=torch.uint8, device=device)
        skip = -self.alloc.data_ptr() % 16  # (a CPU allocation is aligned to 64 bytes, a device one to 256: this is 0)
        assert skip == 0
        body = self.alloc[L.tbase : L.tbase + (L.nbytes - L.tbase) // L.es * L.es].view(dtype)
        self.tv = torch.as_strided(body, L.shape, L.tstrides, body.storage_offset())  # (as_strided's offset counts from the storage's start)
        self.ptr = self.alloc.data_ptr() + L.kbase
        self.strides = L.kstrides
        self.pair = (self.ptr, self.strides)
        bs = tuple(s * L.es for s in L.tstrides[:3])
        B, C, H, W = L.shape
        self.front = torch.as_strided(self.alloc, (B, C, H, GUARD), bs + (1,), self.alloc.storage_offset() + L.tbase - GUARD)
        self.back = torch.as_strided(self.alloc, (B, C, H, GUARD), bs + (1,), self.alloc.storage_offset() + L.tbase + W * L.es)
        self._flips = [d for d, name in ((0, "image_neg"), (2, "pitch_neg")) if L.kind == name]

    def _order(self, t: torch.Tensor) -> torch.Tensor:
        return t.flip(self._flips) if self._flips else t

    def write(self, dense: torch.Tensor) -> "FarView":
        assert tuple(dense.shape) == self.layout.shape and dense.dtype == self.dtype
        self.tv.copy_(self._order(dense.to(self.alloc.device)))
        return self

    def fill(self, value) -> "FarView":
        self.tv.fill_(value)
        return self

    def read(self) -> torch.Tensor:
        return self._order(self.tv).contiguous()

    def fill_guards(self) -> "FarView":
        dev = self.alloc.device
        self.front.copy_(pattern(0, GUARD, dev).expand_as(self.front))
        self.back.copy_(pattern(GUARD, 2 * GUARD, dev).expand_as(self.back))
        return self

    def check_guards(self) -> None:
        dev = self.alloc.device
        for side, g, want in (("front", self.front, pattern(0, GUARD, dev)), ("back", self.back, pattern(GUARD, 2 * GUARD, dev))):
            bad = g != want
            if bool(bad.any()):
                b, c, y, i = (int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"{self.layout.kind}: the {side} guard of torch-view row (image {b}, channel {c}, row {y}) changed at byte {i} "
                                     f"(0x{int(g[b, c, y, i]):02x}, was 0x{int(want[i]):02x}); {int(bad.sum())} guard bytes differ")


def storage_dtype(dtype):
    """uint16 planes travel as the int16 view of the same bits (torch copies and compares those)"""
    return torch.int16 if dtype == torch.uint16 else dtype


def far_view(dense: torch.Tensor, kind: str, misalign: int = 0, big: int | None = None, device=None, write: bool = True) -> FarView:
    """`dense` ([B, C, H, W], any device) inside one large allocation on `device` (default: dense's).  write = False: the view is left
    unwritten (an output), its guards are filled either way."""
    if dense.dtype == torch.uint16:
        dense = dense.view(torch.int16)
    L = far_layout(dense.shape, dense.element_size(), kind, misalign, big)
    v = FarView(L, dense.dtype, dense.device if device is None else device)
    v.fill_guards()
    return v.write(dense) if write else v


# ---- hashed codes -------------------------------------------------------------------------------------------------------------------------
CHUNK = 1 << 26
_MULT = -7046029254386353131  # 0x9E3779B97F4A7C15 as a signed 64-bit integer: 2^64 / the golden ratio, odd


def code_of(g: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    """int64 codes in [lo, hi] of int64 global row indices: bits 40..63 of g * 0x9E3779B97F4A7C15 (mod 2^64), reduced to the range"""
    h = ((g * _MULT) >> 40) & 0xFFFFFF
    return h % (hi - lo + 1) + lo


def hashed_codes(B: int, H: int, device, lo: int, hi: int, out: torch.Tensor | None = None, dtype=torch.uint8) -> torch.Tensor:
    """[B, H] codes of g = b H + row (out: any view of that shape is filled instead), chunks of at most 2^26 elements"""
    out = torch.empty((B, H), dtype=dtype, device=device) if out is None else out
    assert tuple(out.shape) == (B, H)
    for b in range(B):
        for r0 in range(0, H, CHUNK):
            r1 = min(r0 + CHUNK, H)
            g = torch.arange(b * H + r0, b * H + r1, dtype=torch.int64, device=device)
            out[b, r0:r1] = code_of(g, lo, hi).to(out.dtype)
    return out


def lut_check(out: torch.Tensor, codes: torch.Tensor | None, lut: torch.Tensor, chunk: int = CHUNK):
    """out [B, H] against lut[codes] (codes None: against lut[0] everywhere).  -> (number of mismatches, (b, row) of the first or None)"""
    B, H = out.shape
    count, first = 0, None
    for b in range(B):
        for r0 in range(0, H, chunk):
            o = out[b, r0 : r0 + chunk]
            want = lut[0] if codes is None else lut[codes[b, r0 : r0 + chunk].long()]
            ne = o != want
            n = int(ne.sum())
            if n and first is None:
                first = (b, r0 + int(ne.nonzero()[0, 0]))
            count += n
    return count, first


# ---- the long walks -----------------------------------------------------------------------------------------------------------------------
LIMIT31 = 1 << 31
SIDE_MAX = 1 << 28
# entry -> (B, H of the 32-bit branch at its limit, H of the 64-bit branch, luma rows of a work item)
WALKS = {
    "luma": (8, SIDE_MAX - 1, SIDE_MAX, 1),
    "yuv420_to_rgb": (8, SIDE_MAX - 1, SIDE_MAX, 1),
    "rgb_to_yuv420": (16, SIDE_MAX - 2, SIDE_MAX, 2),
    "ycbcr_to_rgb": (8, SIDE_MAX - 1, SIDE_MAX, 1),
    "rgb_to_ycbcr": (8, SIDE_MAX - 1, SIDE_MAX, 1),
}


# branch: 32 (the 32-bit branch at its limit), 64 (the first size of the 64-bit branch: items = 2^31, every item index still fits a signed
# 32-bit integer) or "past" (2^28 items more, one more image -- two where an item is two rows: item indices beyond 2^31 exist, so an `int`
# anywhere in the 64-bit branch shows)
BRANCHES = (32, 64, "past")


def walk_batch(entry: str, branch) -> int:
    B, _, _, per = WALKS[entry]
    return B + per if branch == "past" else B


def walk_items(entry: str, branch) -> int:
    """work items of the W = 1 case of an entry: B * rows, one run a row"""
    _, h32, h64, per = WALKS[entry]
    H = h32 if branch == 32 else h64
    return walk_batch(entry, branch) * ((H + per - 1) // per)


Rows = namedtuple("Rows", "label b r0 r1")  # rows [r0, r1) of image b; r0 is even
BLOCK_ROWS = 64


def walk_blocks(B: int, H: int, per: int = 1, seed: int = 7):
    """Blocks of at most 64 luma rows: the first and last 64 rows of images 0 and B - 1, the rows around every image boundary, the rows
    around the work items 2^31 - 1 and 2^31 (item i: luma rows per * i ..), and 8 seeded random places.  Every block starts on an even row."""
    blocks = {}

    def add(label, b, r0):
        r0 = max(0, min(r0, H - BLOCK_ROWS))
        blk = Rows(label, b, r0 // 2 * 2, min(r0 + BLOCK_ROWS, H))
        blocks.setdefault(blk[1:], blk)

    for b in sorted({0, B - 1}):
        add(f"image {b} first rows", b, 0)
        add(f"image {b} last rows", b, H)
    for b in range(B - 1):
        add(f"before the boundary {b} | {b + 1}", b, H)
        add(f"after the boundary {b} | {b + 1}", b + 1, 0)
    rows = (H + per - 1) // per
    for item in (LIMIT31 - 1, LIMIT31):
        if item < B * rows:
            b, j = divmod(item, rows)
            add(f"item {item}", b, j * per - BLOCK_ROWS // 2)
    g = torch.Generator().manual_seed(seed)
    for i in range(8):
        b, r0 = (int(torch.randint(0, n, (1,), generator=g)) for n in (B, max(1, H - BLOCK_ROWS + 1)))
        add(f"random {i}", b, r0)
    return list(blocks.values())


def block_codes(blk: Rows, H: int, lo: int, hi: int) -> torch.Tensor:
    """the codes of a block's rows, from the hash alone (host, int64)"""
    return code_of(torch.arange(blk.b * H + blk.r0, blk.b * H + blk.r1, dtype=torch.int64), lo, hi)


# ---- the tall noise frame -----------------------------------------------------------------------------------------------------------------
NOISE_H, NOISE_W, NOISE_SIGMA, NOISE_SEED, NOISE_FILL, NOISE_BLOCK = SIDE_MAX, 6, 0.1, 20240229, 128, 4096
TIE_MARGIN = 1e-9  # in units of one uint8 code: nine orders above what two float64 libraries differ by in ln and cos


def noise_blocks(H: int = NOISE_H, W: int = NOISE_W, n: int = NOISE_BLOCK, seed: int = 11, wrap: int = 1 << 32):
    """(label, first within-image element index) of blocks of n elements: the first and last n of every channel, the n before and the n
    after element `wrap` (2^32: where the counter's high word becomes 1), and 8 seeded random blocks of which 4 lie past `wrap`"""
    hw, total = H * W, 3 * H * W
    out = []
    for c in range(3):
        out += [(f"channel {c} first", c * hw), (f"channel {c} last", (c + 1) * hw - n)]
    if total > wrap:
        out += [("before the wrap", wrap - n), ("after the wrap", wrap)]
    g = torch.Generator().manual_seed(seed)
    for i in range(8):
        lo, hi = (wrap, total - n) if (i % 2 and total > wrap + n) else (0, min(wrap, total) - n)
        out.append((f"random {i}", lo + int(torch.randint(0, hi - lo + 1, (1,), generator=g))))
    return out


def noise_normal(i: np.ndarray, seed: int, stream: int = 0, high_word: bool = True) -> np.ndarray:
    """degrade_ref.normal_ref at the element indices i (uint64); high_word = False: what a kernel that dropped the counter's high word
    would draw"""
    i = np.asarray(i, dtype=np.uint64)
    hi = i >> np.uint64(32) if high_word else np.zeros_like(i)
    u = degrade_ref.philox(i & np.uint64(0xFFFFFFFF), hi, stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1 = (u[0].astype(np.float64) + 0.5) / 4294967296.0
    u2 = (u[1].astype(np.float64) + 0.5) / 4294967296.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise_expected(first: int, n: int = NOISE_BLOCK, fill: int = NOISE_FILL, sigma: float = NOISE_SIGMA, seed: int = NOISE_SEED,
                   high_word: bool = True):
    """(uint8 bytes mz_noise stores at within-image elements first .. first + n - 1 of a frame of `fill` bytes, mask of the elements whose
    value lies more than TIE_MARGIN codes from a rounding tie).  The kernel's arithmetic (mz_degrade.h): v = fill / 255 + sigma n, clamped
    to [0, 1], stored as (uint8)(v * 255 + 0.5)."""
    i = np.arange(first, first + n, dtype=np.uint64)
    v = np.clip(fill / 255.0 + sigma * noise_normal(i, seed, 0, high_word), 0.0, 1.0) * 255.0 + 0.5
    frac = v - np.floor(v)
    sure = np.minimum(frac, 1.0 - frac) > TIE_MARGIN
    return v.astype(np.uint8), sure


# ---- the long-walk cases: grey pixels whose code is the hash of their row ---------------------------------------------------------------
# name -> (entry of WALKS, parameters, lo, hi): the codes are hashed into [lo, hi], chosen so that some byte is never stored (the sentinel)
WALK_CASES = {
    "luma-bt601": ("luma", dict(standard="bt601"), 0, 255),
    "luma-full": ("luma", dict(standard="full"), 0, 254),
    "yuv420_to_rgb": ("yuv420_to_rgb", dict(matrix="bt709", range_="limited", siting="left"), 16, 230),
    "rgb_to_yuv420": ("rgb_to_yuv420", dict(matrix="bt601", range_="limited", siting="center"), 0, 255),
    "ycbcr_to_rgb-10bit-422": ("ycbcr_to_rgb", dict(depth=10, align="low", sub="422", matrix="bt2020", range_="limited", siting="left"), 64, 900),
    "rgb_to_ycbcr-8bit-444": ("rgb_to_ycbcr", dict(depth=8, align="low", sub="444", matrix="bt709", range_="limited", siting="center"), 0, 255),
}
WALK_RUNS = [(name, branch) for name in WALK_CASES for branch in BRANCHES]


def walk_shape(name: str, branch: int):
    """(B, H, luma rows of a work item) of a long-walk case"""
    entry = WALK_CASES[name][0]
    _, h32, h64, per = WALKS[entry]
    return walk_batch(entry, branch), (h32 if branch == 32 else h64), per


def walk_mid(name: str) -> int:
    """the chroma code of a grey pixel"""
    return 1 << (WALK_CASES[name][1].get("depth", 8) - 1)


def walk_src_dtype(name: str):
    return torch.int16 if WALK_CASES[name][1].get("depth", 8) > 8 else torch.uint8


def walk_reference(name: str, codes: torch.Tensor) -> dict:
    """What the entry stores for ONE image of width 1 whose rows hold the grey codes `codes` (1-D, int64), from the restatements of
    color_ref / yuv_ref / ycbcr_ref on the CPU: plane name -> 1-D uint8 tensor ("y" of luma; "r", "g", "b"; "y", "cb", "cr")."""
    import color_ref
    import ycbcr_ref
    import yuv_ref

    entry, p, _, _ = WALK_CASES[name]
    n = codes.numel()
    if entry in ("luma", "rgb_to_yuv420", "rgb_to_ycbcr"):
        x = codes.to(torch.uint8).view(1, 1, n, 1).expand(1, 3, n, 1).contiguous()
        if entry == "luma":
            return {"y": color_ref.luma_expected(x, p["standard"], "u8", 0)[0, 0, :, 0]}
        if entry == "rgb_to_yuv420":
            planes = yuv_ref.to_yuv_expected(x, p["matrix"], p["range_"], p["siting"])
        else:
            planes = [torch.from_numpy(a) for a in ycbcr_ref.to_ycbcr_expected(x, p["depth"], p["align"], p["sub"], p["matrix"], p["range_"], p["siting"])]
        return {k: t[0, 0, :, 0] for k, t in zip(("y", "cb", "cr"), planes)}
    if entry == "yuv420_to_rgb":
        y = codes.to(torch.uint8).view(1, 1, n, 1)
        c = torch.full((1, 1, (n + 1) // 2, 1), 128, dtype=torch.uint8)
        rgb = yuv_ref.to_rgb_expected(y, c, c, p["matrix"], p["range_"], p["siting"], "u8", 1)
    else:
        y = codes.numpy().astype(np.uint16).reshape(1, 1, n, 1)
        c = np.full((1, 1, n, 1), walk_mid(name), dtype=np.uint16)
        rgb = ycbcr_ref.to_rgb_expected(y, c, c, p["depth"], p["align"], p["sub"], p["matrix"], p["range_"], p["siting"], "u8", 1)
    return {k: rgb[0, i, :, 0] for i, k in enumerate("rgb")}


def walk_luts(name: str) -> dict:
    """plane name -> the table code -> stored byte over ALL codes of the depth ("cb", "cr": what every grey code gives, asserted to be the
    mid code and kept as a one-entry table)"""
    depth = WALK_CASES[name][1].get("depth", 8)
    ref = walk_reference(name, torch.arange(1 << depth, dtype=torch.int64))
    for k in ("cb", "cr"):
        if k in ref:
            assert bool((ref[k] == walk_mid(name)).all()), (name, k)
            ref[k] = ref[k][:1].clone()
    return ref


def walk_sentinel(name: str, luts: dict) -> int:
    """a byte that no code of [lo, hi] makes the entry store in any plane"""
    _, _, lo, hi = WALK_CASES[name]
    used = set()
    for k, t in luts.items():
        used |= set((t if k in ("cb", "cr") else t[lo : hi + 1]).tolist())
    free = [v for v in (255, 0, 1, 254) if v not in used]
    assert free, f"{name}: every candidate sentinel is a byte the entry stores for a code of [{lo}, {hi}]"
    return free[0]


def walk_outputs(name: str, B: int, H: int, device, sentinel: int) -> dict:
    """the output planes of a case, each [B, rows] uint8 pre-filled with the sentinel ("rgb": one [B, 3, H] tensor)"""
    entry = WALK_CASES[name][0]
    def new(*shape):
        t = torch.empty(shape, dtype=torch.uint8, device=device)
        for b in range(B):  # (no call spans 2^31 elements)
            t[b].fill_(sentinel)
        return t

    if entry == "luma":
        return {"y": new(B, H)}
    if entry.endswith("to_rgb"):
        return {"rgb": new(B, 3, H)}
    hc = (H + 1) // 2 if entry == "rgb_to_yuv420" else H
    return {"y": new(B, H), "cb": new(B, hc), "cr": new(B, hc)}


def walk_planes(outs: dict) -> dict:
    """plane name -> [B, rows] view of the outputs"""
    if "rgb" in outs:
        return {k: outs["rgb"][:, i] for i, k in enumerate("rgb")}
    return outs


def walk_verify(name: str, B: int, H: int, per: int, codes: torch.Tensor, outs: dict, luts: dict, sentinel: int):
    """The checks of one long-walk run: every written plane against its table on the device the planes live on, then the blocks of
    walk_blocks against the restatement on the host.  Raises AssertionError; returns the number of blocks."""
    _, _, lo, hi = WALK_CASES[name]
    planes = walk_planes(outs)
    dev = codes.device
    for k, plane in planes.items():
        chroma = k in ("cb", "cr")
        n, first = lut_check(plane, None if chroma else codes, luts[k].to(dev))
        if n:
            b, row = first
            left = int((plane[b, row] == sentinel))
            raise AssertionError(f"{name}: {n} elements of plane '{k}' differ from the table; first at image {b}, row {row}: got "
                                 f"{int(plane[b, row])}{' (the sentinel: never stored)' if left else ''}")
    blocks = walk_blocks(B, H, per)
    for blk in blocks:
        want_codes = block_codes(blk, H, lo, hi)
        got_codes = codes[blk.b, blk.r0 : blk.r1].cpu().to(torch.int64)
        assert torch.equal(got_codes, want_codes), f"{name}, block '{blk.label}': the input is not the hash of its row"
        ref = walk_reference(name, want_codes)
        for k, plane in planes.items():
            r0, r1 = (blk.r0 // 2, (blk.r1 + 1) // 2) if plane.shape[1] != H else (blk.r0, blk.r1)
            got = plane[blk.b, r0:r1].cpu()
            if not torch.equal(got, ref[k]):
                i = int((got != ref[k]).nonzero()[0, 0])
                raise AssertionError(f"{name}, block '{blk.label}' (image {blk.b}, rows {blk.r0}..{blk.r1 - 1}), plane '{k}': row {r0 + i} holds "
                                     f"{int(got[i])}, the restatement gives {int(ref[k][i])}")
    return len(blocks)
