"""Large-offset test data (tests/test_large_offsets_cpu.py, tests/test_large_offsets_gpu.py).  Needs no GPU.

The 3x3 and mix families address their tensors with 32-bit byte offsets; choose_conv3 / choose_mix (mz_select.h) keep each inside
offsets_fit(planes, pixels), planes * pixels * 16 < 2^32, and hand larger layers to a kernel with wider addressing.  TABLE names, per
family, the smallest shape that sits ON that guard: H is derived (h_fit) from the row's plane count, never typed in.  Every row gives two
cases: "edge" at H_fit (the guarded family, offsets up to just under 2^32) and "past" at H_fit + 1 (the fallback, offsets past 2^32).

Such tensors hold gigabytes, so nothing here builds them on the host.  Inputs are filled ON THE DEVICE with seeded integers (exact_util's
recipe: any fp32 summation order is exact), the whole output is compared bit for bit against a reference computed with plain torch
matmuls in row chunks (sweep), and small blocks -- image corners, the pixels where an offset crosses 2^31 and 2^32, random places -- are
copied to the host and compared with float64 (check_block), which also holds the sweep's own reference to an independent computation.
All of it takes a device argument: the CPU tests run every function below at small shapes before it judges a kernel."""

from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

from exact_util import AW, EXACT_SUM, F16_MAX_OUT, GATE_SCALE, INT_MAX, SAT_HI, SAT_LO, choice, conv_ax, gate_aw, ints, round_once
from gpu_util import DTYPES, F32_OP_TOL, op_excess, pad16, planes_per, ulp_of
from op_cases import ARGS
from oracle import mewzoom_oracle as oracle

LIMIT = 1 << 32

# n: the issue's row number.  entry: "conv" (silu: conv1 + SiLU), "d2s", "conv_mix" (cin: hidden channels), "mix" (cin = cout = C).
# planes x scope: the guard.  scope "image": pixels = H W; "target": the 2H x 2W target image of a sub-pixel conv; "tensor": B H W.
LRow = namedtuple("LRow", "n entry silu cin cout dt B W planes scope edge past")
TABLE = [
    LRow(1, "conv", 0, 96, 96, "bf16", 1, 4075, 12, "image", "conv3r", "conv3s"),
    LRow(2, "conv", 0, 96, 96, "bf16", 1, 4115, 12, "image", "conv3r_8x40", "conv3s"),  # pads to 4120 (8x40) < 4128 (8x48) < 4160 (8x64)
    LRow(3, "conv", 1, 48, 96, "bf16", 2, 4075, 12, "image", "conv3r_ragged", "conv3p"),
    LRow(4, "conv_mix", 0, 192, 96, "bf16", 1, 4075, 12, "image", "conv3r_fused", "conv3s_fused"),
    LRow(5, "d2s", 0, 96, 192, "bf16", 1, 4075, 6, "target", "conv3r", "conv3s"),
    LRow(6, "conv", 0, 96, 48, "bf16", 1, 4093, 6, "image", "conv3t", "conv3s"),
    LRow(7, "conv_mix", 0, 96, 48, "bf16", 1, 4093, 6, "image", "conv3t_fused", "conv3s_fused"),
    LRow(8, "conv", 0, 32, 16, "bf16", 1, 8189, 4, "image", "conv3s", "conv3p"),        # four-plane halo offsets: H W < 2^26
    LRow(9, "conv_mix", 0, 64, 32, "bf16", 1, 8189, 4, "image", "conv3s_fused", "conv3p"),  # "conv3p": the per-tile fused kernel (kernel_name())
    LRow(10, "conv", 0, 16, 16, "bf16", 1, 8189, 2, "image", "conv3p", "conv3w"),
    LRow(11, "conv", 0, 16, 16, "f32", 1, 8189, 2, "image", "conv3p", "conv3w"),         # a stage is two 16-byte planes in every dtype
    LRow(12, "mix", 0, 192, 192, "bf16", 2, 2045, 24, "tensor", "mix16b", "conv_kernel_mix"),
    LRow(13, "mix", 0, 384, 384, "bf16", 2, 2045, 48, "tensor", "mix16", "conv_kernel_mix"),
]
F16_TOO = (1, 12)  # these rows run once more in f16, at H_fit


def guard_pixels(row: LRow, H: int) -> int:
    return {"image": 1, "target": 4, "tensor": row.B}[row.scope] * H * row.W


def h_fit(row: LRow) -> int:
    """The largest H for which row.planes * pixels * 16 < 2^32."""
    per_row = row.planes * 16 * guard_pixels(row, 1)
    return (LIMIT - 1) // per_row


# One GPU case.  kernel: what mz_debug_last_kernel() must report (None: the entry reports none).
Case = namedtuple("Case", "name entry silu cin cout dt B H W kernel kind")


def _cases():
    out = []
    for r in TABLE:
        H = h_fit(r)
        out.append(Case(f"row{r.n}-{r.entry}-{r.cin}to{r.cout}-{r.dt}-edge", r.entry, r.silu, r.cin, r.cout, r.dt, r.B, H, r.W, r.edge, "edge"))
        if r.n in F16_TOO:
            out.append(Case(f"row{r.n}-{r.entry}-{r.cin}to{r.cout}-f16-edge", r.entry, r.silu, r.cin, r.cout, "f16", r.B, H, r.W, r.edge, "edge"))
        out.append(Case(f"row{r.n}-{r.entry}-{r.cin}to{r.cout}-{r.dt}-past", r.entry, r.silu, r.cin, r.cout, r.dt, r.B, H + 1, r.W, r.past, "past"))
    # entries outside the guarded families (long long addressing by design), the fewest channels, one tensor past 2^32 bytes:
    # the stem's output and the 2x2 conv's input are 16 channels = 32 B per pixel, the head's dense output 3 x 4 x 2 B per conv pixel
    W = 8189
    Hs = LIMIT // (32 * W) + 1
    out.append(Case("stem-3to16-bf16-past", "stem", 0, 3, 16, "bf16", 1, Hs, W, None, "past"))
    out.append(Case("crush-16to16-bf16-past", "crush", 0, 16, 16, "bf16", 1, Hs, W, None, "past"))
    out.append(Case("final-16-R2-bf16-past", "final", 0, 16, 12, "bf16", 1, LIMIT // (24 * W) + 1, W, "conv_kernel", "past"))
    return out


CASES = _cases()
FINAL_R = 2
FINAL_W_SCALE = 2.0 ** -10  # the head's weights: integers times 2^-10, so that the conv term does not bury the bicubic skip in [0, 1]


def op_args(c, H=None):
    """The argument tuple (op_cases.ARGS) of a Case, or of an LRow at height H."""
    H = c.H if H is None else H
    v = dict(B=c.B, H=H, W=c.W, cin=c.cin, cout=c.cout, C=c.cout, silu=c.silu, Hout=2 * H, Wout=2 * c.W, R=FINAL_R)
    return tuple(v[n] for n in ARGS[c.entry] if n in v)


# ---- offset spaces and blocks ---------------------------------------------------------------------------------------------------------
def crossing(planes: int, H: int, W: int, bound: int, unit: int = 16):
    """The first (plane, y, x) of a [planes, H, W] space of `unit`-byte elements whose offset ((p H + y) W + x) unit reaches `bound`;
    None where no offset does."""
    idx = -(-bound // unit)
    if idx >= planes * H * W:
        return None
    p, r = divmod(idx, H * W)
    return (p, *divmod(r, W))


BH, BW = 16, 256  # a block: at most 16 rows x 256 columns (plus the one-pixel halo)
Block = namedtuple("Block", "label b y0 x0 h w")  # in conv-grid pixels (the 2x2 conv: output pixels)
# P planes of Hs x Ws `unit`-byte elements per image; grid pixel = space pixel // scale
Space = namedtuple("Space", "name P Hs Ws unit scale")


def grid_of(c: Case):
    return (c.H // 2, c.W // 2) if c.entry == "crush" else (c.H, c.W)


def spaces(c: Case):
    """The offset spaces of a case: every tensor as the kernel may address it."""
    u = 16 // planes_per(DTYPES[c.dt])  # bytes of one element
    pin, pout = pad16(c.cin) * u // 16, pad16(c.cout) * u // 16
    H, W = c.H, c.W
    if c.entry == "conv":
        return [Space("halo", 4, H, W, 16, 1), Space("in", pin, H, W, 16, 1), Space("store", pout, H, W, 16, 1)]
    if c.entry == "d2s":
        return [Space("halo", 4, H, W, 16, 1), Space("in", pin, H, W, 16, 1), Space("store", pout // 4, 2 * H, 2 * W, 16, 2)]
    if c.entry == "conv_mix":
        return [Space("halo", 4, H, W, 16, 1), Space("hid", pin, H, W, 16, 1), Space("x", pout, H, W, 16, 1), Space("store", pout, H, W, 16, 1)]
    if c.entry == "mix":
        return [Space("x", pout, H, W, 16, 1)]  # z and the output: the same space
    if c.entry == "stem":
        return [Space("img", 3, H, W, u, 1), Space("store", pout, H, W, 16, 1)]
    if c.entry == "crush":
        return [Space("in", pin, H, W, 16, 2), Space("store", pout, H // 2, W // 2, 16, 1)]
    if c.entry == "final":
        return [Space("feat", pin, H, W, 16, 1), Space("img", 3, 2 * H // FINAL_R, 2 * W // FINAL_R, u, 2 // FINAL_R), Space("store", 3, 2 * H, 2 * W, u, 2)]
    raise ValueError(c.entry)


def _clamp(v, lo, hi):
    return max(lo, min(v, hi))


def pick_blocks(c: Case, seed: int = 7):
    """Corners of every image, the block around and the block before every crossing of 2^31 (and of 2^32 where one exists) in every
    offset space -- inside the last image, and along the whole tensor where B > 1 --, and 8 seeded random blocks."""
    GH, GW = grid_of(c)
    h, w = min(BH, GH), min(BW, GW)
    blocks = {}

    def add(label, b, y0, x0):
        blk = Block(label, b, _clamp(y0, 0, GH - h), _clamp(x0, 0, GW - w), h, w)
        blocks.setdefault(blk[1:], blk)

    for b in range(c.B):
        for cy, y0 in (("top", 0), ("bottom", GH - h)):
            for cx, x0 in (("left", 0), ("right", GW - w)):
                add(f"image {b} {cy} {cx}", b, y0, x0)
    for sp in spaces(c):
        for whole in ((False, True) if c.B > 1 else (False,)):
            planes = sp.P * c.B if whole else sp.P
            for bound in (1 << 31, 1 << 32):
                at = crossing(planes, sp.Hs, sp.Ws, bound, sp.unit)
                if at is None:
                    continue
                idx = (at[0] * sp.Hs + at[1]) * sp.Ws + at[2]
                p, y, x = at
                b = p // sp.P if whole else c.B - 1
                add(f"{sp.name} crosses 2^{bound.bit_length() - 1}", b, min(y // sp.scale, GH - 1) - h // 2, min(x // sp.scale, GW - 1) - w // 2)
                if idx:
                    p, r = divmod(idx - 1, sp.Hs * sp.Ws)
                    y, x = divmod(r, sp.Ws)
                    b = p // sp.P if whole else c.B - 1
                    add(f"{sp.name} before 2^{bound.bit_length() - 1}", b, min(y // sp.scale, GH - 1) - h + 1, min(x // sp.scale, GW - 1) - w + 1)
    g = torch.Generator().manual_seed(seed)
    for i in range(8):
        b, y0, x0 = (int(torch.randint(0, n, (1,), generator=g)) for n in (c.B, GH - h + 1, GW - w + 1))
        add(f"random {i}", b, y0, x0)
    return list(blocks.values())


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def alloc(B, C, H, W, dtype, fill=7.0, device="cpu"):
    """gpu_util.alloc_act on any device."""
    ppu = planes_per(dtype)
    return torch.full((B, pad16(C) // ppu, H, W, ppu), fill, dtype=dtype, device=device)


def to_layout(x: torch.Tensor, dtype, device="cpu"):
    """gpu_util.to_act on any device: [B, C, H, W] -> [B, P, H, W, channels per plane], pad channels zero."""
    B, C, H, W = x.shape
    ppu = planes_per(dtype)
    t = torch.zeros(B, pad16(C), H, W, dtype=dtype, device=device)
    t[:, :C] = x.to(device=device, dtype=dtype)
    return t.reshape(B, pad16(C) // ppu, ppu, H, W).permute(0, 1, 3, 4, 2).contiguous()


def chw(t4: torch.Tensor) -> torch.Tensor:
    """[P, h, w, channels per plane] (rows / columns of one image) -> [P * ppu, h, w]."""
    P, h, w, u = t4.shape
    return t4.permute(0, 3, 1, 2).reshape(P * u, h, w)


def checksum(t: torch.Tensor) -> int:
    """64-bit wrapping sum of the tensor's bit pattern, eight bytes at a time (no temporary: the view is summed as it lies)."""
    raw = t.reshape(-1).view(torch.uint8)
    n8 = raw.numel() // 8 * 8
    return int(raw[:n8].view(torch.int64).sum()) + int(raw[n8:].sum(dtype=torch.int64))


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def amplitudes(c: Case) -> dict:
    """Worst-case bounds of a case's data: activations in [-ax, ax] (mix: x in [-ax, ax], z multiples of 4 in [-4 az, 4 az]), 3x3 / 2x2
    weights in [-AW, AW]; `conv`: the largest sum of absolute products a convolution can reach, which must stay below 2^24."""
    big = c.dt == "f16" or bool(c.silu)
    if c.entry in ("conv", "d2s", "conv_mix", "final"):
        ax = conv_ax(9 * c.cin, c.dt, big)
        a = {"ax": ax, "conv": 9 * c.cin * ax * AW}
        if c.entry == "conv_mix":
            # x = k + 1/2, |k + 1/2| <= 127.5 (8 significant bits: a bf16 value).  z is an integer, so x + z and 3 x + z are never zero:
            # where the gate is 16 or 0 the blend (x + z) / 2, (3 x + z) / 4 cannot cancel to (almost) nothing, which is where an fp32
            # evaluation leaves the one-operator tolerance (soft_error_bound(); EXPERIMENTS.md section 18)
            assert c.dt == "bf16"
            a["xx"] = 127.5
        return a
    if c.entry == "crush":
        return {"ax": 15, "conv": 4 * c.cin * 15 * AW}
    if c.entry == "mix":
        # Small on purpose: the fp32 evaluation error of the soft elements, soft_error_bound(), then stays below the tolerance's absolute
        # floor of 1e-5 whatever cancels: with w <= 1/2 and |z - x| <= 27, 2^-24 (15 + 8 x 1/2 x 27) = 7.3e-6.  EXPERIMENTS.md section 18 has the
        # measurement behind it.
        return {"ax": 15, "az": 3, "gate": c.cout * (15 + 12) * GATE_SCALE * AW}
    return {"ax": INT_MAX[c.dt], "conv": 3 * INT_MAX[c.dt] * 2 + 8}  # stem: |w| <= 2, |b| <= 8


def _fill(t: torch.Tensor, lo: int, hi: int, gen, scale: int = 1):
    """Seeded integers of [lo, hi] in the storage type, slab by slab (one image plane at a time: no call spans 2^32 elements), from
    ONE generator sequence -- no block of data ever repeats."""
    flat = t.reshape(t.shape[0] * t.shape[1], -1)
    for i in range(flat.shape[0]):
        flat[i].random_(lo, hi + 1, generator=gen)
    if scale != 1:
        t.mul_(scale)
    return t


def make_inputs(c: Case, device="cpu", alloc_act=None, seed: int = 1234):
    """The case's tensors by argument name, in the library's layout on `device`, filled there; weights are built on the host
    (exact_util.ints) and travel as float32.  alpha is 0 for every mix: sigmoid(0) = 1/2 exactly."""
    dtype = DTYPES[c.dt]
    mk = alloc_act or (lambda B, C, H, W, dt: alloc(B, C, H, W, dt, device=device))
    gen = torch.Generator(device=device).manual_seed(seed)
    dev = lambda w: w.to(device, torch.float32).contiguous()
    a = amplitudes(c)
    B, H, W = c.B, c.H, c.W
    if c.entry in ("conv", "d2s", "crush"):
        k = 2 if c.entry == "crush" else 3
        return {"in0": _fill(mk(B, c.cin, H, W, dtype), -a["ax"], a["ax"], gen), "w": dev(ints((c.cout, c.cin, k, k), AW, 102))}
    if c.entry == "conv_mix":
        hid = _fill(mk(B, c.cin, H, W, dtype), -a["ax"], a["ax"], gen)
        x = _fill(mk(B, c.cout, H, W, dtype), -128, 127, gen).add_(0.5)
        mean_z = 0.8 * (9 * c.cin) ** 0.5 * a["ax"] * AW / 3.0  # as exact_util
        wmix = ints((c.cout, 2 * c.cout, 1, 1), gate_aw(c.cout, a["xx"] / 2.0, mean_z), 115, float(GATE_SCALE))
        return {"hid": hid, "x": x, "w2": dev(ints((c.cout, c.cin, 3, 3), AW, 114)), "wmix": dev(wmix)}
    if c.entry == "mix":
        x = _fill(mk(B, c.cout, H, W, dtype), -a["ax"], a["ax"], gen)
        z = _fill(mk(B, c.cout, H, W, dtype), -a["az"], a["az"], gen, 4)
        wmix = ints((c.cout, 2 * c.cout, 1, 1), gate_aw(c.cout, a["ax"] / 2.0, 2.0 * a["az"]), 115, float(GATE_SCALE))
        return {"in0": x, "in1": z, "w": dev(wmix)}
    if c.entry == "stem":
        x = _fill(torch.empty(B, 3, H, W, dtype=dtype, device=device), 0, a["ax"], gen)
        return {"x": x, "w": dev(choice((c.cout, 3, 1, 1), [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], 106)), "b": dev(ints((c.cout,), 8, 107))}
    if c.entry == "final":
        feat = _fill(mk(B, c.cin, H, W, dtype), -a["ax"], a["ax"], gen)
        img = torch.empty(B, 3, 2 * H // FINAL_R, 2 * W // FINAL_R, dtype=dtype, device=device)
        for b in range(B):
            for ch in range(3):
                img[b, ch].uniform_(0.0, 1.0, generator=gen)
        return {"feat": feat, "img": img, "w": dev(ints((12, c.cin, 3, 3), AW, 109, FINAL_W_SCALE))}
    raise ValueError(c.entry)


def out_shape(c: Case):
    """(channels or None for a dense image, shape of the output tensor)."""
    dtype = DTYPES[c.dt]
    ppu = planes_per(dtype)
    if c.entry == "final":
        return None, (c.B, 3, 2 * c.H, 2 * c.W)
    C = c.cout // 4 if c.entry == "d2s" else c.cout
    H, W = (2 * c.H, 2 * c.W) if c.entry == "d2s" else grid_of(c)
    return C, (c.B, pad16(C) // ppu, H, W, ppu)


# ---- the sweep: the whole output against fp32 matmuls, bit for bit ----------------------------------------------------------------------
def _conv3_rows(xb: torch.Tensor, w: torch.Tensor, y0: int, y1: int) -> torch.Tensor:
    """3x3, pad 1, rows [y0, y1) of one image xb [P, H, W, ppu]: nine shifted [cout, cin] @ [cin, pixels] fp32 matmuls over the
    zero-padded rows (exact in any order on this data).  -> [cout, y1 - y0, W] float32"""
    H, W = xb.shape[1:3]
    cout, cin = w.shape[:2]
    lo, hi = max(y0 - 1, 0), min(y1 + 1, H)
    x = F.pad(chw(xb[:, lo:hi])[:cin].float(), (1, 1, lo - (y0 - 1), (y1 + 1) - hi))
    h = y1 - y0
    acc = torch.zeros(cout, h * W, dtype=torch.float32, device=xb.device)
    for ky in range(3):
        for kx in range(3):
            acc.addmm_(w[:, :, ky, kx], x[:, ky:ky + h, kx:kx + W].reshape(cin, h * W))
    return acc.reshape(cout, h, W)


def _mix_rows(x, z, wmix, dtype):
    """AdaptiveResidualMix at alpha = 0 on exact data: x, z [C, h, W] float32 (storage-type values).  -> (what is rounded, mask of the
    elements whose gate lies inside (SAT_LO, SAT_HI), the float64 formula there, the gate's largest sum of absolute products)"""
    C = x.shape[0]
    xz = torch.cat([x, z]).reshape(2 * C, -1)
    w = wmix.reshape(C, 2 * C)
    gate = (w @ xz).reshape(x.shape)
    abs_sum = (w.abs() @ xz.abs_()).max()
    del xz
    hi, lo = gate >= SAT_HI, gate <= SAT_LO
    y = torch.where(hi, (x + z) / 2, x)
    soft = ~(hi | lo)
    xs, zs = x[soft].double(), z[soft].double()
    w = 0.5 * torch.sigmoid(gate[soft].double())
    return y, soft, xs + w * (zs - xs), abs_sum, soft_error_bound(xs, zs, w)


SOFT_ROUNDINGS = 8


def soft_error_bound(x64, z64, w64):
    """What an fp32 evaluation of x + w (z - x) may err by: z - x is exact (integers, or integers + 1/2), w = sigmoid(alpha) sigmoid(gate)
    comes out of an exponential, a reciprocal, a sum and products -- at most SOFT_ROUNDINGS roundings of 2^-24 relative with the
    product w (z - x) --, the final sum rounds once more at the larger of |x| and |w (z - x)|.  A condition on the DATA: the sweep asserts
    that it lies inside the one-operator tolerance of every soft element, so that no correct fp32 kernel can miss that tolerance."""
    p = (w64 * (z64 - x64)).abs()
    return 2.0 ** -24 * (x64.abs() + SOFT_ROUNDINGS * p)


def reference_rows(c: Case, t: dict, b: int, y0: int, y1: int):
    """Grid rows [y0, y1) of image b.  -> (first output row, want [C, rows, width] in the storage type, soft mask or None, float64
    values at the soft elements or None, {quantity: largest sum of absolute products, as a tensor})"""
    dtype = DTYPES[c.dt]
    soft = soft64 = None
    sums = {}
    oy = y0
    if c.entry in ("conv", "d2s"):
        y = _conv3_rows(t["in0"][b], t["w"], y0, y1)
        if c.entry == "d2s":
            y, oy = F.pixel_shuffle(y[None], 2)[0], 2 * y0
        elif c.silu:
            hi, lo = y >= SAT_HI, y <= SAT_LO
            soft = ~(hi | lo)
            soft64 = F.silu(y[soft].double())
            y = torch.where(hi, y, torch.zeros_like(y))
    elif c.entry == "conv_mix":
        z = _conv3_rows(t["hid"][b], t["w2"], y0, y1).to(dtype).float()  # z is rounded to the storage type before the gate and the blend
        x = chw(t["x"][b][:, y0:y1])[:c.cout].float()
        y, soft, soft64, sums["gate"], bound = _mix_rows(x, z, t["wmix"], dtype)
    elif c.entry == "mix":
        x, z = (chw(t[k][b][:, y0:y1])[:c.cout].float() for k in ("in0", "in1"))
        y, soft, soft64, sums["gate"], bound = _mix_rows(x, z, t["w"], dtype)
    elif c.entry == "stem":
        W = t["x"].shape[3]
        y = torch.addmm(t["b"][:, None], t["w"].reshape(c.cout, 3), t["x"][b][:, y0:y1].reshape(3, -1).float()).reshape(c.cout, y1 - y0, W)
    elif c.entry == "crush":
        GH, GW = grid_of(c)
        x = chw(t["in0"][b][:, 2 * y0:2 * y1, :2 * GW])[:c.cin].float()
        y = torch.zeros(c.cout, (y1 - y0) * GW, dtype=torch.float32, device=x.device)
        for ky in range(2):
            for kx in range(2):
                y.addmm_(t["w"][:, :, ky, kx], x[:, ky::2, kx::2].reshape(c.cin, -1))
        y = y.reshape(c.cout, y1 - y0, GW)
    else:
        raise ValueError(c.entry)
    sums["out"] = y.abs().max()
    if c.entry in ("mix", "conv_mix") and bound.numel():
        # the data's own condition: bound / tolerance of the element (gpu_util.op_excess's denominator), from the reference alone
        tol = ulp_of(soft64.float(), c.dt).double() + 1e-5 if c.dt != "f32" else torch.full_like(bound, F32_OP_TOL)
        sums["soft_bound"] = (bound / tol).max()
    return oy, y.to(dtype), soft, soft64, sums


class Report:
    """What a sweep saw: elements compared for equality / differing, non-finite elements of the whole chunk (pad channels included),
    non-zero pad-channel elements, elements excluded (soft), their worst |got - want| / tolerance, the first difference in words."""

    def __init__(self):
        self.total = self.differ = self.nonfinite = self.nan = self.pad_nonzero = self.soft = 0
        self.soft_excess = 0.0
        self.first = None
        self.sums = {}

    @property
    def excluded(self) -> float:
        return self.soft / max(1, self.total + self.soft)


CHUNK_ELEMS = 48 << 20  # fp32 elements of the widest tensor of a chunk: temporaries of a few hundred MB each


def chunk_rows(c: Case) -> int:
    GW = grid_of(c)[1]
    widest = max(2 * c.cout if c.entry in ("mix", "conv_mix") else c.cout, c.cin)
    return max(1, CHUNK_ELEMS // (widest * GW))


def whole_tensor_counts(out: torch.Tensor, rows: int, rep: Report):
    """NaN / non-finite elements of a dense output, in row chunks."""
    for b in range(out.shape[0]):
        for y0 in range(0, out.shape[2], rows):
            o = out[b, :, y0:y0 + rows]
            rep.nan += int(torch.isnan(o).sum())
            rep.nonfinite += int((~torch.isfinite(o)).sum())


def sweep(c: Case, t: dict, out: torch.Tensor, rows: int | None = None) -> Report:
    """The whole output against reference_rows, chunk by chunk, on the device the tensors live on."""
    rep = Report()
    C, _ = out_shape(c)
    GH, _ = grid_of(c)
    rows = rows or chunk_rows(c)
    for b in range(c.B):
        for y0 in range(0, GH, rows):
            y1 = min(y0 + rows, GH)
            oy, want, soft, soft64, sums = reference_rows(c, t, b, y0, y1)
            got_all = chw(out[b][:, oy:oy + want.shape[1]])
            got, pad = got_all[:C], got_all[C:]
            assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
            rep.nan += int(torch.isnan(got_all).sum())
            rep.nonfinite += int((~torch.isfinite(got_all)).sum())
            rep.pad_nonzero += int((pad != 0).sum())
            ne = got != want
            if soft is not None:
                ne &= ~soft
                n_soft = int(soft.sum())
                rep.soft += n_soft
                if n_soft:
                    g = got[soft]
                    if bool(torch.isfinite(g).all()):
                        rep.soft_excess = max(rep.soft_excess, op_excess(g, soft64.float(), c.dt))
                    else:
                        rep.soft_excess = float("inf")
            else:
                n_soft = 0
            rep.total += want.numel() - n_soft
            n = int(ne.sum())
            if n and rep.first is None:
                ch, y, x = (int(v) for v in ne.nonzero()[0])
                rep.first = (f"image {b} channel {ch} output row {oy + y} column {x}: got {got[ch, y, x].item()!r}, want {want[ch, y, x].item()!r} "
                             f"({n} differ in rows {oy}..{oy + want.shape[1] - 1})")
            rep.differ += n
            for k, v in sums.items():
                rep.sums[k] = max(rep.sums.get(k, 0.0), float(v))
    return rep


def assert_report(c: Case, rep: Report, max_excluded: float):
    assert rep.nan == 0, f"{c.name}: {rep.nan} NaN left in the output: a dropped store"
    assert rep.nonfinite == 0, f"{c.name}: {rep.nonfinite} non-finite output elements"
    assert rep.pad_nonzero == 0, f"{c.name}: {rep.pad_nonzero} pad-channel elements are not zero"
    assert rep.sums.get("gate", 0.0) < EXACT_SUM, f"{c.name}: the gate's sums reach {rep.sums['gate']}: the data are not exact"
    if c.dt == "f16":
        assert rep.sums["out"] <= F16_MAX_OUT, f"{c.name}: outputs reach {rep.sums['out']}"
    assert rep.sums.get("soft_bound", 0.0) <= 1.0, (f"{c.name}: the DATA let an fp32 evaluation of an excluded element err by "
                                                    f"{rep.sums['soft_bound']:.2f} x the one-operator tolerance")
    assert rep.differ == 0, f"{c.name}: {rep.differ} of {rep.total} elements differ from the reference rounded once; first: {rep.first}"
    assert rep.excluded <= max_excluded, f"{c.name}: excluded share {rep.excluded:.5f}"
    assert rep.soft_excess <= 1.0, f"{c.name}: excluded elements reach {rep.soft_excess:.2f} x the one-operator tolerance"


# ---- blocks: float64 on the host ----------------------------------------------------------------------------------------------------------
def _window(tb: torch.Tensor, C: int, ylo: int, yhi: int, xlo: int, xhi: int) -> torch.Tensor:
    """Rows [ylo, yhi) x columns [xlo, xhi) of one image [P, H, W, ppu] as float64 [1, C, rows, columns] on the host; what lies outside
    the image is zero."""
    H, W = tb.shape[1:3]
    a, b_, l, r = max(ylo, 0), min(yhi, H), max(xlo, 0), min(xhi, W)
    x = chw(tb[:, a:b_, l:r].cpu())[:C].double()
    return F.pad(x, (l - xlo, xhi - r, a - ylo, yhi - b_))[None]


def block_expectation(c: Case, t: dict, blk: Block):
    """-> (what is rounded: float64 [C, rows, columns] of the OUTPUT block, output row, output column, mask of the elements compared
    for equality or None, the float64 formula for the others or None)"""
    d = lambda w: w.detach().cpu().double()
    b, y0, x0, h, w = blk.b, blk.y0, blk.x0, blk.h, blk.w
    y1, x1 = y0 + h, x0 + w
    keep = soft64 = None
    oy, ox = y0, x0
    if c.entry in ("conv", "d2s"):
        y = F.conv2d(_window(t["in0"][b], c.cin, y0 - 1, y1 + 1, x0 - 1, x1 + 1), d(t["w"]))
        if c.entry == "d2s":
            y, oy, ox = F.pixel_shuffle(y, 2), 2 * y0, 2 * x0
        elif c.silu:
            hi, lo = y >= SAT_HI, y <= SAT_LO
            keep, soft64 = hi | lo, F.silu(y)
            y = torch.where(hi, y, torch.zeros_like(y))
    elif c.entry in ("conv_mix", "mix"):
        if c.entry == "mix":
            x, z = (_window(t[k][b], c.cout, y0, y1, x0, x1) for k in ("in0", "in1"))
            wmix = d(t["w"])
        else:
            z = F.conv2d(_window(t["hid"][b], c.cin, y0 - 1, y1 + 1, x0 - 1, x1 + 1), d(t["w2"]))
            z = round_once(z, c.dt).double()
            x, wmix = _window(t["x"][b], c.cout, y0, y1, x0, x1), d(t["wmix"])
        gate = F.conv2d(torch.cat([x, z], dim=1), wmix)
        hi, lo = gate >= SAT_HI, gate <= SAT_LO
        keep, soft64 = hi | lo, x + 0.5 * torch.sigmoid(gate) * (z - x)
        y = torch.where(hi, (x + z) / 2, x)
    elif c.entry == "stem":
        y = F.conv2d(t["x"][b:b + 1, :, y0:y1, x0:x1].cpu().double(), d(t["w"]), d(t["b"]))
    elif c.entry == "crush":
        y = F.conv2d(_window(t["in0"][b], c.cin, 2 * y0, 2 * y1, 2 * x0, 2 * x1), d(t["w"]), stride=2)
    elif c.entry == "final":
        assert FINAL_R == 2
        conv = F.pixel_shuffle(F.conv2d(_window(t["feat"][b], c.cin, y0 - 1, y1 + 1, x0 - 1, x1 + 1), d(t["w"])), 2)
        # bicubic x 2: output pixel 2 k + p reads k - 2 .. k + 2, clamped to the image.  Two more source pixels on every side, or the
        # image's own edge, and the crop leaves exactly the pixels whose taps the window holds
        Hi, Wi = t["img"].shape[2:]
        ylo, yhi, xlo, xhi = max(y0 - 2, 0), min(y1 + 2, Hi), max(x0 - 2, 0), min(x1 + 2, Wi)
        up = oracle.bicubic_upsample(t["img"][b:b + 1, :, ylo:yhi, xlo:xhi].cpu().double(), 2)
        y = conv + up[:, :, 2 * (y0 - ylo):2 * (y0 - ylo) + 2 * h, 2 * (x0 - xlo):2 * (x0 - xlo) + 2 * w]
        oy, ox = 2 * y0, 2 * x0
    else:
        raise ValueError(c.entry)
    return y[0], oy, ox, None if keep is None else keep[0], None if soft64 is None else soft64[0]


def block_of_output(c: Case, out: torch.Tensor, blk: Block, oy: int, ox: int, rows: int, cols: int):
    """(real channels, pad channels) of the output block on the host, in the storage type."""
    C, _ = out_shape(c)
    if C is None:
        return out[blk.b, :, oy:oy + rows, ox:ox + cols].cpu(), None
    g = chw(out[blk.b][:, oy:oy + rows, ox:ox + cols].cpu())
    return g[:C], g[C:]


def check_block(c: Case, t: dict, out: torch.Tensor, blk: Block):
    """One block against float64 on the host: equality after one rounding (the head, whose bicubic skip is not exact, and the elements
    inside the transcendental's window: the one-operator tolerance).  Raises AssertionError; returns the number of soft elements."""
    y64, oy, ox, keep, soft64 = block_expectation(c, t, blk)
    got, pad = block_of_output(c, out, blk, oy, ox, y64.shape[1], y64.shape[2])
    where = f"{c.name}, block '{blk.label}' (image {blk.b}, output rows {oy}.., columns {ox}..)"
    assert got.shape == y64.shape, (got.shape, y64.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{where}: non-finite output"
    if pad is not None:
        assert bool((pad == 0).all()), f"{where}: pad channels are not zero"
    if c.entry == "final":
        ex = op_excess(got, y64.float(), c.dt)
        assert ex <= 1.0, f"{where}: |got - want| reaches {ex:.2f} x (1 ulp + 1e-5)"
        return 0
    want = round_once(y64, c.dt)
    bad = (got != want) if keep is None else (got != want) & keep
    if bool(bad.any()):
        ch, y, x = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{where}: {int(bad.sum())} of {bad.numel()} elements differ from float64 rounded once; first at channel {ch}, "
                             f"row {oy + y}, column {ox + x}: got {got[ch, y, x].item()!r}, want {want[ch, y, x].item()!r}")
    if keep is None or bool(keep.all()):
        return 0
    soft = ~keep
    ex = op_excess(got[soft], soft64[soft].float(), c.dt)
    assert ex <= 1.0, f"{where}: excluded elements reach {ex:.2f} x (1 ulp + 1e-5)"
    return int(soft.sum())
