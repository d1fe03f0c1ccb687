"""The large-offset table and its helpers (tests/large_util.py) without a GPU: the table against the host's choice on both sides of every
guard, the block picker against brute force, the data's worst-case bounds, and the sweep reference -- run on the CPU device at small
shapes -- against exact_util's float64 expectation, bit for bit.  tests/test_large_offsets_gpu.py lets these helpers judge kernels; here
they are shown to agree with an independent computation and to report a wrong or an unwritten element."""

import pytest
import torch

import large_util as lu
from exact_util import AW, EXACT_SUM, F16_MAX_OUT, INT_MAX, MAX_EXCLUDED, Row, bits_of, exact
from gpu_util import DTYPES
from op_util import selected, set_knobs
from oracle import mewzoom_oracle as oracle

LIMIT = 1 << 32


def chosen(dt, c, H):
    return selected(c.entry, lu.op_args(c, H), dt)


@pytest.fixture
def no_knobs(monkeypatch):
    set_knobs(monkeypatch)


@pytest.mark.parametrize("row", lu.TABLE, ids=lambda r: f"row{r.n}")
def test_the_table_sits_on_the_host_s_guards(row, no_knobs):
    """H_fit is the exact edge of planes * pixels * 16 < 2^32 for the row's plane count; the host chooses the row's family there and its
    fallback one row further.  A change to a guard in mz_select.h fails here and names its row."""
    pixels = {"image": lambda H: H * row.W, "target": lambda H: 2 * H * 2 * row.W, "tensor": lambda H: row.B * H * row.W}[row.scope]
    H = lu.h_fit(row)
    assert row.planes * pixels(H) * 16 < LIMIT <= row.planes * pixels(H + 1) * 16
    assert H > 16 and pixels(H) * 16 > (1 << 31) // row.planes  # offsets between 2^31 and 2^32 exist
    assert chosen(row.dt, row, H) == row.edge
    assert chosen(row.dt, row, H + 1) == row.past
    if row.n in lu.F16_TOO:
        assert chosen("f16", row, H) == row.edge
    # the plane count is the tensor's own where the guard is about stores (and about x, z for the mix)
    u = torch.empty((), dtype=DTYPES[row.dt]).element_size()
    if row.planes not in (2, 4):  # 4: conv3s's halo planes; 2: a stage of conv3p
        assert row.planes == (row.cout // 4 if row.entry == "d2s" else row.cout) * u // 16


def test_the_cases_cover_both_sides_of_every_row():
    by_kind = {k: [c for c in lu.CASES if c.kind == k] for k in ("edge", "past")}
    assert len(by_kind["edge"]) == len(lu.TABLE) + len(lu.F16_TOO) and len(by_kind["past"]) == len(lu.TABLE) + 3
    assert len({c.name for c in lu.CASES}) == len(lu.CASES)
    assert {c.kernel for c in by_kind["edge"]} == {"conv3r", "conv3r_8x40", "conv3r_ragged", "conv3r_fused", "conv3t", "conv3t_fused", "conv3s",
                                                   "conv3s_fused", "conv3p", "mix16", "mix16b"}
    for c in lu.CASES:
        nbytes = {k: v.numel() * v.element_size() for k, v in meta_tensors(c).items()}
        assert sum(nbytes.values()) < 18e9, (c.name, nbytes)  # + the sweep's temporaries: below 20 GB
        if c.kind == "past":
            assert max(nbytes.values()) > LIMIT, (c.name, nbytes)


def meta_tensors(c):
    """Sizes only: the case's tensors as make_inputs / out_shape shape them, on the meta device."""
    t = {}
    dtype = DTYPES[c.dt]
    if c.entry in ("conv", "d2s", "crush"):
        t["in0"] = lu.alloc(c.B, c.cin, c.H, c.W, dtype, device="meta")
    elif c.entry == "conv_mix":
        t["hid"], t["x"] = lu.alloc(c.B, c.cin, c.H, c.W, dtype, device="meta"), lu.alloc(c.B, c.cout, c.H, c.W, dtype, device="meta")
    elif c.entry == "mix":
        t["in0"] = lu.alloc(c.B, c.cout, c.H, c.W, dtype, device="meta")
        t["in1"] = lu.alloc(c.B, c.cout, c.H, c.W, dtype, device="meta")
    elif c.entry == "stem":
        t["x"] = torch.empty(c.B, 3, c.H, c.W, dtype=dtype, device="meta")
    else:
        t["feat"] = lu.alloc(c.B, c.cin, c.H, c.W, dtype, device="meta")
        t["img"] = torch.empty(c.B, 3, 2 * c.H // lu.FINAL_R, 2 * c.W // lu.FINAL_R, dtype=dtype, device="meta")
    t["out"] = torch.empty(lu.out_shape(c)[1], dtype=dtype, device="meta")
    return t


def test_the_head_s_case_runs_the_256_pixel_kernel(no_knobs):
    c = next(c for c in lu.CASES if c.entry == "final")
    assert chosen(c.dt, c, c.H) == c.kernel


@pytest.mark.parametrize("space", [(1, 3, 5, 16), (4, 7, 9, 16), (3, 6, 4, 2), (5, 1, 11, 16), (2, 9, 1, 4)])
def test_crossing_against_brute_force(space):
    planes, H, W, unit = space
    offsets = [(((p * H + y) * W + x) * unit, (p, y, x)) for p in range(planes) for y in range(H) for x in range(W)]
    for bound in list(range(0, planes * H * W * unit + 2 * unit, 3)) + [planes * H * W * unit - 1, planes * H * W * unit]:
        want = next((at for off, at in offsets if off >= bound), None)
        assert lu.crossing(planes, H, W, bound, unit) == want, (space, bound)


@pytest.mark.parametrize("case", lu.CASES, ids=lambda c: c.name)
def test_blocks_lie_inside_the_image_and_on_the_crossings(case):
    GH, GW = lu.grid_of(case)
    blocks = lu.pick_blocks(case)
    assert 4 * case.B + 8 <= len(blocks) <= 4 * case.B + 8 + 4 * 2 * 2 * 4  # (a crossing that falls on a plane's first pixel IS a corner)
    for blk in blocks:
        assert 0 <= blk.b < case.B and 0 <= blk.y0 and blk.y0 + blk.h <= GH and 0 <= blk.x0 and blk.x0 + blk.w <= GW
        assert blk.h <= lu.BH and blk.w <= lu.BW
    assert any(b.b == case.B - 1 and b.y0 + b.h == GH and b.x0 + b.w == GW for b in blocks)  # the largest offsets
    # some block holds the pixel of every crossing, another the pixel before it
    crossed = set()
    for sp in lu.spaces(case):
        for planes in {sp.P, sp.P * case.B}:  # inside the last image; along the whole tensor
            for bound in (1 << 31, 1 << 32):
                at = lu.crossing(planes, sp.Hs, sp.Ws, bound, sp.unit)
                if at is None:
                    continue
                crossed.add(bound)
                idx = (at[0] * sp.Hs + at[1]) * sp.Ws + at[2]
                for i in (idx, idx - 1):
                    p, r = divmod(i, sp.Hs * sp.Ws)
                    y, x = divmod(r, sp.Ws)
                    y, x, b = min(y // sp.scale, GH - 1), min(x // sp.scale, GW - 1), case.B - 1 if planes == sp.P else p // sp.P
                    assert any(k.b == b and k.y0 <= y < k.y0 + k.h and k.x0 <= x < k.x0 + k.w for k in blocks), (sp, bound, i)
    assert (1 << 31) in crossed and ((1 << 32) in crossed or case.kind == "edge"), crossed


@pytest.mark.parametrize("case", lu.CASES, ids=lambda c: c.name)
def test_data_bounds_are_worst_case(case):
    """Every activation is an integer the storage type holds, and the largest sum of absolute products any convolution of the case can
    reach -- every activation at +-ax, every weight at +-AW -- stays below 2^24: fp32 adds such data without error in any order."""
    a = lu.amplitudes(case)
    assert a["ax"] <= INT_MAX[case.dt] and a.get("xx", 0) <= INT_MAX[case.dt]
    if "conv" in a:
        assert a["conv"] < EXACT_SUM
    if case.entry in ("conv", "d2s", "conv_mix") and not (case.silu or case.dt == "f16"):
        assert a["ax"] == 15 and a["conv"] == 9 * case.cin * 15 * AW
    if case.entry == "mix":
        assert a["gate"] < EXACT_SUM  # the gate's sum, every term at its largest
        # the soft elements: large_util.soft_error_bound at its largest, 2^-24 (15 + 8 x 1/2 x 27) = 7.3e-6, lies below the tolerance's floor of 1e-5
        assert 2.0 ** -24 * (a["ax"] + lu.SOFT_ROUNDINGS * 0.5 * (a["ax"] + 4 * a["az"])) < 1e-5
    if case.dt == "f16" and case.entry == "conv":
        assert a["conv"] > F16_MAX_OUT  # not bounded by the worst case: the GPU test asserts the output maximum on the device


# ---- the sweep on the CPU device ---------------------------------------------------------------------------------------------------------
# one row of each kind at a small shape: (entry, exact_util arguments, dtype, silu)
SMALL = [("conv", (2, 13, 37, 96, 96, 0), "bf16", 0), ("conv", (1, 13, 37, 96, 96, 0), "f16", 0), ("conv", (1, 9, 33, 16, 16, 0), "f32", 0),
         ("d2s", (1, 12, 37, 96, 192, 24, 74), "bf16", 0), ("conv", (2, 13, 37, 48, 96, 1), "bf16", 1), ("mix", (2, 11, 29, 192), "bf16", 0),
         ("mix", (1, 11, 29, 192), "f16", 0), ("conv_mix", (2, 13, 37, 192, 96), "bf16", 0), ("stem", (2, 9, 11, 16), "bf16", 0),
         ("crush", (1, 21, 19, 16, 16), "bf16", 0)]


def small_case(entry, args, dt, silu):
    B, H, W = args[:3]
    cin, cout = (args[3], args[3]) if entry == "mix" else (3, args[3]) if entry == "stem" else args[3:5]
    return lu.Case("small-" + entry, entry, silu, cin, cout, dt, B, H, W, None, "small")


def from_exact(entry, args, dt, silu):
    """exact_util's data of a small row in the library's layout on the CPU device, and its expectation as an output tensor."""
    ex = exact(Row(entry, tuple(args), {}, dt, None, silu))
    c = small_case(entry, args, dt, silu)
    dtype = DTYPES[dt]
    t = {}
    for name, v in ex.inputs.items():
        if name in ("in0", "in1", "hid", "feat") or (name == "x" and entry != "stem"):
            t[name] = lu.to_layout(v, dtype)
        elif name == "x":
            t[name] = v.to(dtype)
        else:
            t[name] = v.float()
    # exact_util's expectation holds a placeholder where the transcendental is not exact: an output has the formula's value there
    want = ex.want if ex.keep is None else torch.where(ex.keep, ex.want, ex.soft64.float().to(dtype))
    return c, ex, t, lu.to_layout(want.float(), dtype)


@pytest.mark.parametrize("small", SMALL, ids=lambda s: f"{s[0]}-{s[2]}" + ("-silu" if s[3] else ""))
def test_the_sweep_equals_the_float64_expectation_bit_for_bit(small):
    """reference_rows -- fp32 matmuls, one torch rounding, in chunks of 5 rows so that chunk seams lie inside the image -- against
    exact_util's float64 expectation rounded on the bit pattern; the elements it excludes are exact_util's, at most MAX_EXCLUDED."""
    c, ex, t, out = from_exact(*small)
    assert lu.op_args(c) == tuple(small[1])
    rep = lu.sweep(c, t, out, rows=5)
    lu.assert_report(c, rep, MAX_EXCLUDED)
    assert rep.total + rep.soft == ex.want.numel()
    assert rep.soft == (0 if ex.keep is None else int((~ex.keep).sum()))
    assert rep.excluded == pytest.approx(ex.excluded) and rep.excluded <= MAX_EXCLUDED
    if "gate" in ex.sums:
        assert rep.sums["gate"] == ex.sums["gate"]
    # and the default chunking (one chunk here) gives the same verdict
    rep1 = lu.sweep(c, t, out)
    assert (rep1.total, rep1.differ, rep1.soft) == (rep.total, 0, rep.soft)
    # the blocks' float64 path, on the same tensors
    for blk in lu.pick_blocks(c):
        lu.check_block(c, t, out, blk)


@pytest.mark.parametrize("small", [SMALL[0], SMALL[3], SMALL[5], SMALL[7]], ids=lambda s: s[0])
def test_the_sweep_reports_a_wrong_and_an_unwritten_element(small):
    """A copy of the expectation with ONE element one storage-type step off, then with one left as NaN: the sweep reports each, and
    so does the block that holds it."""
    c, ex, t, good = from_exact(*small)
    keep = torch.ones_like(ex.want, dtype=torch.bool) if ex.keep is None else ex.keep
    b, ch, y, x = (int(v) for v in keep.nonzero()[len(keep.nonzero()) // 2])  # an element that is compared for equality
    ppu = good.shape[-1]
    at = (b, ch // ppu, y, x, ch % ppu)
    off = good.clone()
    bits_of(off)[at] += 1
    rep = lu.sweep(c, t, off, rows=5)
    assert (rep.differ, rep.nan, rep.nonfinite) == (1, 0, 0) and f"image {b} channel {ch} output row {y} column {x}:" in rep.first
    with pytest.raises(AssertionError, match="1 of .* elements differ"):
        lu.assert_report(c, rep, MAX_EXCLUDED)
    unwritten = good.clone()
    unwritten[at] = float("nan")
    rep = lu.sweep(c, t, unwritten, rows=5)
    assert (rep.differ, rep.nan, rep.nonfinite) == (1, 1, 1)
    with pytest.raises(AssertionError, match="1 NaN left in the output"):
        lu.assert_report(c, rep, MAX_EXCLUDED)
    GH, GW = lu.grid_of(c)
    s = 2 if c.entry == "d2s" else 1
    blk = lu.Block("the element", b, min(y // s, GH - 1), min(x // s, GW - 1), 1, 1)
    lu.check_block(c, t, good, blk)
    for bad in (off, unwritten):
        with pytest.raises(AssertionError):
            lu.check_block(c, t, bad, blk)
    # an input that changes is seen by the checksum
    before = lu.checksum(t[next(iter(t))])
    bits_of(t[next(iter(t))]).view(-1)[3] ^= 1
    assert lu.checksum(t[next(iter(t))]) != before
    bits_of(t[next(iter(t))]).view(-1)[3] ^= 1
    assert lu.checksum(t[next(iter(t))]) == before


# ---- the cases' own data, filled on the (CPU) device ---------------------------------------------------------------------------------------
OWN = [lu.Case("own-conv", "conv", 0, 96, 96, "bf16", 2, 21, 300, None, "small"), lu.Case("own-silu", "conv", 1, 48, 96, "bf16", 1, 21, 300, None, "small"),
       lu.Case("own-d2s", "d2s", 0, 96, 192, "bf16", 1, 21, 300, None, "small"), lu.Case("own-conv_mix", "conv_mix", 0, 64, 32, "bf16", 2, 21, 300, None, "small"),
       lu.Case("own-mix", "mix", 0, 192, 192, "f16", 2, 21, 300, None, "small"), lu.Case("own-stem", "stem", 0, 3, 16, "bf16", 1, 21, 300, None, "small"),
       lu.Case("own-crush", "crush", 0, 16, 16, "bf16", 1, 21, 301, None, "small"), lu.Case("own-conv-f32", "conv", 0, 16, 16, "f32", 1, 21, 300, None, "small")]


@pytest.mark.parametrize("case", OWN, ids=lambda c: c.name)
def test_device_filled_data_meet_their_bounds_and_both_references_agree(case):
    """make_inputs on the CPU device: integers inside the stated amplitudes, no two images alike; an output assembled from the sweep's
    reference passes every float64 block, the excluded share stays below MAX_EXCLUDED."""
    t = lu.make_inputs(case, "cpu")
    a = lu.amplitudes(case)
    for name, v in t.items():
        f = v.float()
        if case.entry == "conv_mix" and name == "x":  # k + 1/2: x + z and 3 x + z are never zero (large_util.amplitudes)
            assert bool(((2 * f) % 2 == 1).all()) and f.abs().max().item() == a["xx"]
        else:
            assert bool((f == f.round()).all()) or name in ("w",) and case.entry == "stem", name
    x = t[{"conv": "in0", "d2s": "in0", "crush": "in0", "conv_mix": "hid", "mix": "in0", "stem": "x"}[case.entry]].float()
    assert x.abs().max().item() == a["ax"] and (case.entry == "stem" or x.min().item() == -a["ax"])
    if case.B > 1:
        assert not torch.equal(x[0], x[1])
    C, shape = lu.out_shape(case)
    out = torch.full(shape, float("nan"), dtype=DTYPES[case.dt])
    GH, _ = lu.grid_of(case)
    for b in range(case.B):
        for y0 in range(0, GH, 8):
            oy, want, soft, soft64, _ = lu.reference_rows(case, t, b, y0, min(y0 + 8, GH))
            if soft is not None:
                want[soft] = soft64.float().to(want.dtype)
            ppu = shape[-1]
            out[b][:, oy:oy + want.shape[1]] = want.reshape(C // ppu, ppu, *want.shape[1:]).permute(0, 2, 3, 1)
    rep = lu.sweep(case, t, out)
    lu.assert_report(case, rep, MAX_EXCLUDED)
    blocks = lu.pick_blocks(case)
    soft = sum(lu.check_block(case, t, out, blk) for blk in blocks)
    assert (soft > 0) == (rep.soft > 0) or rep.excluded < 1e-4


def test_the_head_s_blocks_against_the_whole_image_oracle():
    """The head is compared on blocks only: a block's expectation -- bicubic skip from a cropped window -- equals the whole image's."""
    case = lu.Case("own-final", "final", 0, 16, 12, "bf16", 2, 21, 300, "conv_kernel", "small")
    t = lu.make_inputs(case, "cpu")
    assert 0.0 <= t["img"].float().min().item() and t["img"].float().max().item() <= 1.0 and t["img"].float().std().item() > 0.2
    feat = torch.stack([lu.chw(t["feat"][b]) for b in range(case.B)]).double()
    whole = oracle.bicubic_upsample(t["img"].double(), 2) + oracle.subpixel_conv(feat, t["w"].double())
    assert whole.abs().max().item() < 64  # the conv term does not bury the image
    for blk in lu.pick_blocks(case):
        y64, oy, ox, keep, _ = lu.block_expectation(case, t, blk)
        assert keep is None and torch.allclose(y64, whole[blk.b, :, oy:oy + 2 * blk.h, ox:ox + 2 * blk.w], rtol=0, atol=1e-12)
        lu.check_block(case, t, whole.to(DTYPES[case.dt]), blk)
    rep = lu.Report()
    bad = whole.to(DTYPES[case.dt])
    bad[1, 2, 5, 7] = float("nan")
    lu.whole_tensor_counts(bad, 16, rep)
    assert (rep.nan, rep.nonfinite) == (1, 1)
