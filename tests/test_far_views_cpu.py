"""tests/far_util.py held to non-vacuity, without a GPU: the far views lie where they claim, the hashed codes tell a decode error from the
truth, lut_check and the block picker find one planted wrong byte where the long walks could go wrong, the sizes of the long walks are
the items they claim, and the noise blocks can show a dropped counter word."""

import numpy as np
import pytest
import torch

import far_util as fu
from ultrazoom_amd import _ffi

ES = {torch.uint8: 1, torch.int16: 2, torch.bfloat16: 2, torch.float32: 4}
SMALL = {"image": 1 << 14, "image_neg": 1 << 14, "channel": 1 << 13, "pitch": 1 << 11, "pitch_neg": 1 << 11}  # reduced large strides, bytes


# ---- far_view: geometry at reduced strides -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1, 3])
@pytest.mark.parametrize("dtype", list(ES), ids=str)
@pytest.mark.parametrize("kind", fu.KINDS)
def test_far_view_reads_back_the_dense_tensor_and_guards_sit_where_claimed(kind, dtype, misalign):
    B, C, H, W = (2 if kind.startswith("image") else 1), 3, 5, 21
    g = torch.Generator().manual_seed(3)
    dense = torch.randint(0, 200, (B, C, H, W), generator=g).to(dtype)
    v = fu.far_view(dense, kind, misalign, big=SMALL[kind])
    L, es = v.layout, ES[dtype]
    v.alloc.copy_(torch.full_like(v.alloc, 0xEE))
    v.fill_guards().write(dense)
    assert torch.equal(v.read(), dense)
    # the KERNEL's addressing: element (b, c, y, x) at kbase + (b s0 + c s1 + y s2 + x s3) es, read straight from the allocation's bytes
    raw = v.alloc.numpy()
    flat = dense.view(torch.uint8 if es == 1 else torch.int16 if es == 2 else torch.int32).numpy()
    np_t = {1: np.uint8, 2: np.int16, 4: np.int32}[es]
    owned = np.zeros(raw.size, dtype=bool)
    for b in range(B):
        for c in range(C):
            for y in range(H):
                at = L.kbase + (b * L.kstrides[0] + c * L.kstrides[1] + y * L.kstrides[2]) * es
                assert 0 <= at - fu.GUARD and at + W * es + fu.GUARD <= raw.size
                assert np.array_equal(raw[at : at + W * es].view(np_t), flat[b, c, y])
                want = fu.pattern(0, 2 * fu.GUARD, "cpu").numpy()
                assert np.array_equal(raw[at - fu.GUARD : at], want[: fu.GUARD]) and np.array_equal(raw[at + W * es : at + W * es + fu.GUARD], want[fu.GUARD :])
                assert not owned[at - fu.GUARD : at + W * es + fu.GUARD].any(), "rows or guards overlap"
                owned[at - fu.GUARD : at + W * es + fu.GUARD] = True
    assert bool((raw[~owned] == 0xEE).all()), "something outside the rows and their guards was written"
    v.check_guards()
    assert v.ptr == v.alloc.data_ptr() + L.kbase and v.strides == L.kstrides
    # a stray byte in any guard is found
    for where in (L.tbase - 1, L.tbase + W * es, L.kbase + W * es + fu.GUARD - 1):
        keep = int(v.alloc[where])
        v.alloc[where] = keep ^ 0x40
        with pytest.raises(AssertionError, match="guard"):
            v.check_guards()
        v.alloc[where] = keep
    v.check_guards()


# ---- far_view: the offsets at the real strides, nothing allocated -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(ES), ids=str)
@pytest.mark.parametrize("kind", fu.KINDS)
def test_far_offsets_cross_the_bounds_they_name(kind, dtype):
    es = ES[dtype]
    B, C, H, W = (2 if kind.startswith("image") else 1), 3, fu.PITCH_H, 258
    L0, L1 = fu.far_layout((B, C, H, W), es, kind, 0), fu.far_layout((B, C, H, W), es, kind, 1)
    assert L0.nbytes < fu.MAX_DEVICE_BYTES and L1.nbytes < fu.MAX_DEVICE_BYTES
    off = np.abs(fu.element_offsets(L0))  # bytes from the kernel's pointer, [B, C, H]
    if kind.startswith("image"):
        assert abs(L0.kstrides[0]) >= (1 << 31) + 40 and (L0.kstrides[0] < 0) == (kind == "image_neg")
        assert off[1, 0, 0] > (1 << 31) * es and off[0].max() < 1 << 31
        if kind == "image":
            assert off[1].min() > (1 << 31) * es
        else:  # the rows of image 1 lie AFTER its first element: their negative offsets come back towards -2^31 by the image's own extent
            assert fu.element_offsets(L0)[1].max() < -(1 << 31) * es + C * H * 2048
    elif kind == "channel":
        assert L0.kstrides[1] * es == (1 << 32) + 64
        assert off[0, 1].min() > 1 << 32 and off[0, 2].min() > 1 << 33
        if es == 2:  # the 16-bit types: ELEMENT offsets past 2^31 (channel 1) and 2^32 (channel 2)
            assert off[0, 1].min() // es > 1 << 31 and off[0, 2].min() // es > 1 << 32
    else:
        assert abs(L0.kstrides[2]) * es == (1 << 28) + 64 and (L0.kstrides[2] < 0) == (kind == "pitch_neg")
        ch = slice(0, C) if kind == "pitch" else slice(0, 1)  # (bottom-up, the channels beside channel 0 lie a few hundred bytes back towards 0)
        assert off[0, :, 7].max() < 1 << 31 and off[0, ch, 8].min() > 1 << 31
        assert off[0, :, 15].max() < 1 << 32 and off[0, ch, 16].min() > 1 << 32 and off[0, ch, 17].min() > 1 << 32
    # misalign = 0: the base and every stride of a dimension that steps are multiples of 16 bytes; misalign = 1 breaks base and large stride
    steps = [d for d, n in enumerate((B, C, H)) if n > 1]
    assert L0.kbase % 16 == 0 and all(L0.kstrides[d] * es % 16 == 0 for d in steps)
    large = {"image": 0, "image_neg": 0, "channel": 1, "pitch": 2, "pitch_neg": 2}[kind]
    assert L1.tbase % 16 == es and L1.kbase % 16 != 0 and abs(L1.kstrides[large]) * es % 16 == es
    # torch's view and the kernel's name the same bytes
    for L in (L0, L1):
        t = L.tbase + np.array([(B - 1) * L.tstrides[0], (H - 1) * L.tstrides[2]]) * es
        assert L.kbase in (L.tbase, int(t[0]), int(t[1])) and L.tbase - fu.GUARD >= 0
        lo = L.kbase + sum(min(0, (n - 1) * s) for n, s in zip(L.shape, L.kstrides)) * es
        hi = L.kbase + (sum(max(0, (n - 1) * s) for n, s in zip(L.shape, L.kstrides)) + 1) * es
        assert lo == L.tbase and hi + fu.GUARD <= L.nbytes


@pytest.mark.parametrize("dtype", list(ES), ids=str)
def test_view_extent_accepts_every_far_view(dtype):
    """mz_blur takes its two views through check_views and check_overlap -- view_extent (mz_view_check.h) of both -- before it looks at
    sigma: with a negative sigma and addresses that are never dereferenced, a far view whose byte range view_extent accepts reaches the
    sigma refusal, and two far views over the same bytes are refused as overlapping."""
    from ctypes import byref

    es, elem = ES[dtype], {torch.float32: 0, torch.bfloat16: 1, torch.int16: 2, torch.uint8: 3}[dtype]
    lib = _ffi.lib()
    for kind in fu.KINDS:
        for misalign in (0, 1):
            B, H, W = (2 if kind.startswith("image") else 1), fu.PITCH_H, 258
            L = fu.far_layout((B, 3, H, W), es, kind, misalign)
            x, out = _ffi.view((1 << 40) + L.kbase, L.kstrides), _ffi.view((1 << 45) + L.kbase, L.kstrides)
            code = lib.mz_blur(byref(x), byref(out), elem, B, H, W, -1.0, None)
            assert code == _ffi.MZ_ERR_INVALID_ARGUMENT and lib.mz_last_error().decode().startswith("sigma -1"), (kind, misalign, lib.mz_last_error())
            shifted = _ffi.view((1 << 40) + L.kbase + 16 * es, L.kstrides)
            code = lib.mz_blur(byref(x), byref(shifted), elem, B, H, W, -1.0, None)
            assert code == _ffi.MZ_ERR_INVALID_ARGUMENT and "overlap" in lib.mz_last_error().decode(), (kind, misalign, lib.mz_last_error())


# ---- hashed codes -------------------------------------------------------------------------------------------------------------------------
def test_hashed_codes_are_the_hash_of_the_global_row_chunk_by_chunk(monkeypatch):
    monkeypatch.setattr(fu, "CHUNK", 1000)  # several chunks, a ragged last one
    B, H = 3, 2501
    got = fu.hashed_codes(B, H, "cpu", 16, 230)
    g = torch.arange(B * H, dtype=torch.int64)
    assert got.dtype == torch.uint8 and torch.equal(got.reshape(-1).long(), fu.code_of(g, 16, 230))
    assert int(got.min()) == 16 and int(got.max()) == 230
    out = torch.zeros((B, H + 3), dtype=torch.int16)[:, :H]
    assert fu.hashed_codes(B, H, "cpu", 64, 900, out=out) is out and int(out.min()) == 64 and int(out.max()) == 900
    # the multiplication wraps modulo 2^64 as written: against Python integers
    for v in (0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, 16 * (1 << 28) - 1):
        want = (((v * 0x9E3779B97F4A7C15) % (1 << 64)) >> 40) % 215 + 16
        assert int(fu.code_of(torch.tensor([v]), 16, 230)) == want, v


@pytest.mark.parametrize("lo, hi", [(0, 255), (0, 254), (16, 230), (64, 900)])
def test_hashed_codes_tell_a_decode_error_from_the_truth(lo, hi):
    """On 2^22 sampled positions of the case with the most rows whose H is no power of two (B = 16, H = 2^28 - 2: with H = 2^28 a wrapped
    b H leaves the row as it is) the codes of g and of what a decode error would read agree at
    most at 1 % of the positions (a random code collides at 1 / 256)."""
    B, H = 16, fu.SIDE_MAX - 2
    g = torch.randint(0, B * H, (1 << 22,), generator=torch.Generator().manual_seed(1), dtype=torch.int64)
    g[:4] = torch.tensor([0, B * H - 1, (1 << 31) - 1, 1 << 31])
    b, row = g // H, g % H
    wrapped = (b.to(torch.int32) * torch.tensor(H, dtype=torch.int32)).to(torch.int64)  # b * H as a 32-bit product
    wrong = {
        "g + 1": g + 1, "g - 1": g - 1, "g + H": g + H, "g - H": g - H, "g mod 2^31": g % (1 << 31), "g mod 2^32": g % (1 << 32),
        "row from a wrapped b H": b * H + (g - wrapped) % H, "b H wrapped": wrapped + row, "b from a wrapped b H": ((wrapped + row) // H) * H + row,
    }
    truth = fu.code_of(g, lo, hi)
    for what, w in wrong.items():
        differs = w != g
        if what == "g mod 2^32":  # B H = 2^32 at most: no row index of these cases reaches it, the shift is the identity
            assert not bool(differs.any())
            continue
        assert int(differs.sum()) > (1 << 20), what  # the error is one: it moves at least a quarter of the samples
        share = float((fu.code_of(w, lo, hi)[differs] == truth[differs]).double().mean())
        assert share <= 0.01, (what, share)


# ---- lut_check, the block picker, the whole verification ------------------------------------------------------------------------------------
def test_lut_check_counts_and_places_mismatches(monkeypatch):
    lut = torch.arange(255, -1, -1, dtype=torch.uint8)
    codes = fu.hashed_codes(2, 700, "cpu", 0, 255)
    out = lut[codes.long()]
    assert fu.lut_check(out, codes, lut, chunk=256) == (0, None)
    for b, row in ((0, 0), (1, 699), (1, 256), (0, 255)):
        bad = out.clone()
        bad[b, row] ^= 1
        assert fu.lut_check(bad, codes, lut, chunk=256) == (1, (b, row))
    bad = out.clone()
    bad[1, 5] ^= 1
    bad[0, 699] ^= 1
    assert fu.lut_check(bad, codes, lut, chunk=256) == (2, (0, 699))
    still = torch.full((2, 700), 128, dtype=torch.uint8)
    assert fu.lut_check(still, None, torch.tensor([128], dtype=torch.uint8)) == (0, None)
    still[1, 3] = 127
    assert fu.lut_check(still, None, torch.tensor([128], dtype=torch.uint8)) == (1, (1, 3))
    # a strided plane (one channel of an RGB tensor)
    rgb = torch.stack([out, out, out], dim=1)
    assert fu.lut_check(rgb[:, 1], codes, lut, chunk=256) == (0, None)


def test_the_long_walks_have_the_items_they_claim():
    assert {e: fu.walk_items(e, 32) for e in fu.WALKS} == {"luma": 2**31 - 8, "yuv420_to_rgb": 2**31 - 8, "rgb_to_yuv420": 2**31 - 16,
                                                           "ycbcr_to_rgb": 2**31 - 8, "rgb_to_ycbcr": 2**31 - 8}
    assert all(fu.walk_items(e, 64) == 2**31 and fu.walk_items(e, "past") == 2**31 + 2**28 for e in fu.WALKS)
    assert {e: fu.walk_batch(e, "past") for e in fu.WALKS} == {"luma": 9, "yuv420_to_rgb": 9, "rgb_to_yuv420": 18, "ycbcr_to_rgb": 9, "rgb_to_ycbcr": 9}
    assert all(fu.walk_items(e, "past") * 256 // 256 <= 0xFFFFFFFF for e in fu.WALKS)  # (a grid dimension holds them: 2^32 - 1 work-items)
    for e, (B, h32, h64, per) in fu.WALKS.items():
        assert h64 == fu.SIDE_MAX and B <= 65535 and B * -(-h32 // per) <= 0x7FFFFFFF < B * -(-h64 // per)
    assert {name: fu.walk_shape(name, 64)[:2] for name in fu.WALK_CASES}["rgb_to_yuv420"] == (16, 2**28)


@pytest.mark.parametrize("B, H, per", [(8, 2**28 - 1, 1), (8, 2**28, 1), (9, 2**28, 1), (16, 2**28 - 2, 2), (16, 2**28, 2), (18, 2**28, 2), (3, 100, 1), (2, 31, 2)])
def test_walk_blocks_cover_the_places_a_walk_can_go_wrong(B, H, per):
    blocks = fu.walk_blocks(B, H, per)
    rows = -(-H // per)

    def covered(b, r):
        return any(k.b == b and k.r0 <= r < k.r1 for k in blocks)

    assert all(0 <= k.r0 < k.r1 <= H and k.r0 % 2 == 0 and k.r1 - k.r0 <= fu.BLOCK_ROWS + 1 and 0 <= k.b < B for k in blocks)
    for b in (0, B - 1):
        assert covered(b, 0) and covered(b, min(63, H - 1)) and covered(b, H - 1) and covered(b, max(0, H - 64))
    for b in range(B - 1):
        assert covered(b, H - 1) and covered(b + 1, 0)
    for item in ((1 << 31) - 1, 1 << 31):
        if item < B * rows:
            b, j = divmod(item, rows)
            assert all(covered(b, r) for r in range(j * per, min(j * per + per, H))), item
    assert H < 1000 or sum(k.label.startswith("random") for k in blocks) >= 7  # (two seeded places may coincide; a small image is one block)


def fake_run(name, B, H, codes, sentinel):
    """the outputs a correct kernel leaves: the restatement on every image"""
    outs = fu.walk_outputs(name, B, H, "cpu", sentinel)
    planes = fu.walk_planes(outs)
    for b in range(B):
        for k, v in fu.walk_reference(name, codes[b].to(torch.int64)).items():
            planes[k][b] = v
    return outs


@pytest.mark.parametrize("name", list(fu.WALK_CASES))
def test_walk_verify_passes_the_restatement_and_finds_one_planted_byte(name, monkeypatch):
    """The functions of the GPU test at a small shape: 5 images of 203 rows, the item "2^31" moved to 300 so that its row exists."""
    monkeypatch.setattr(fu, "LIMIT31", 300)
    monkeypatch.setattr(fu, "CHUNK", 128)
    entry, _, lo, hi = fu.WALK_CASES[name]
    B, H, per = 5, 203, fu.WALKS[entry][3]
    luts = fu.walk_luts(name)
    sentinel = fu.walk_sentinel(name, luts)
    for k, t in luts.items():
        assert sentinel not in set((t if k in ("cb", "cr") else t[lo : hi + 1]).tolist())
    codes = fu.hashed_codes(B, H, "cpu", lo, hi, dtype=fu.walk_src_dtype(name))
    outs = fake_run(name, B, H, codes, sentinel)
    assert fu.walk_verify(name, B, H, per, codes, outs, luts, sentinel) >= 10
    rows = -(-H // per)
    b31, j31 = divmod(300, rows)
    for k, plane in fu.walk_planes(outs).items():
        scale = 1 if plane.shape[1] == H else 2
        for b, row in ((0, 0), (B - 1, plane.shape[1] - 1), (b31, j31 * per // scale), (2, plane.shape[1] // 3)):
            keep = int(plane[b, row])
            plane[b, row] = keep ^ 1
            with pytest.raises(AssertionError, match="differ from the table"):
                fu.walk_verify(name, B, H, per, codes, outs, luts, sentinel)
            plane[b, row] = keep
        # a store that never happened leaves the sentinel
        keep = int(plane[1, 7])
        plane[1, 7] = sentinel
        with pytest.raises(AssertionError, match="sentinel"):
            fu.walk_verify(name, B, H, per, codes, outs, luts, sentinel)
        plane[1, 7] = keep
    # the blocks alone (a table that is wrong in the same way as the kernel would hide nothing from them)
    lying = {k: t.clone() for k, t in luts.items()}
    first = next(iter(fu.walk_planes(outs)))
    code0 = int(codes[0, 0]) if first not in ("cb", "cr") else 0
    lying[first][code0] ^= 1
    plane = fu.walk_planes(outs)[first]
    hit = codes[:, : plane.shape[1]].long() == code0 if first not in ("cb", "cr") else torch.ones_like(plane, dtype=torch.bool)
    plane[hit] = lying[first][code0]
    with pytest.raises(AssertionError, match="restatement"):
        fu.walk_verify(name, B, H, per, codes, outs, lying, sentinel)


def test_a_32_bit_row_term_fails_the_walk(monkeypatch):
    """What a planted truncation does: a kernel whose row index passed through 32 bits with the scaled-down limit (items modulo 512) stores
    the rows of another place; the table check names the first such row."""
    monkeypatch.setattr(fu, "LIMIT31", 512)
    name, B, H = "luma-bt601", 5, 203
    luts = fu.walk_luts(name)
    sentinel = fu.walk_sentinel(name, luts)
    codes = fu.hashed_codes(B, H, "cpu", 0, 255)
    outs = fake_run(name, B, H, codes, sentinel)
    g = torch.arange(B * H)
    outs["y"].view(-1)[:] = luts["y"][codes.view(-1)[g % 512].long()]  # item g reads the row of item g mod 512
    with pytest.raises(AssertionError, match=r"image 2, row 10[6-9]"):  # 512 = 2 * 203 + 106: the first rows whose hash differs
        fu.walk_verify(name, B, H, 1, codes, outs, luts, sentinel)


# ---- noise ----------------------------------------------------------------------------------------------------------------------------------
def test_noise_blocks_lie_where_the_counter_matters_and_can_show_a_dropped_word():
    H, W, n = fu.NOISE_H, fu.NOISE_W, fu.NOISE_BLOCK
    total, hw = 3 * H * W, H * W
    assert (1 << 32) < total < 2 * (1 << 32) and 2 * hw < (1 << 32) < total, "element 2^32 lies in channel 2"
    blocks = dict(fu.noise_blocks())
    assert len(blocks) == 16 and all(0 <= f and f + n <= total for f in blocks.values())
    assert blocks["before the wrap"] + n == blocks["after the wrap"] == 1 << 32
    assert [blocks[f"channel {c} first"] for c in range(3)] == [0, hw, 2 * hw] and blocks["channel 2 last"] + n == total
    past = [f for f in blocks.values() if f >= 1 << 32]
    assert len(past) >= 6
    for label, first in blocks.items():
        want, sure = fu.noise_expected(first)
        assert bool(sure.all()), f"{label}: an element lies within {fu.TIE_MARGIN} codes of a rounding tie"
        assert 100 < len(set(want.tolist())) or fu.NOISE_SIGMA < 0.05  # noise, not a constant
        if first >= 1 << 32:
            # the reference itself: the block at i and the block at i - 2^32 differ, as do the bytes a dropped high word would give
            earlier, _ = fu.noise_expected(first - (1 << 32))
            dropped, _ = fu.noise_expected(first, high_word=False)
            assert np.array_equal(earlier, dropped)
            assert int((earlier != want).sum()) > n // 2, label
    # noise_normal is degrade_ref.normal_ref at the same indices
    import degrade_ref

    assert np.array_equal(fu.noise_normal(np.arange(50), fu.NOISE_SEED, 3), degrade_ref.normal_ref(50, fu.NOISE_SEED, 3))
