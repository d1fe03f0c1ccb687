"""Every operator entry and every kernel family in poisoned surroundings (tests/poison_util.py).

The parity tests give each tensor a fresh allocation of its own; nothing there checks WHERE a kernel reads and writes.  Here every
row of CASES runs three times:
  (a) on ordinary tensors: the family that ran (mz_debug_last_kernel) and the oracle, as the parity tests assert them;
  (b) with every device pointer carved from an Arena -- inputs and weights between NaN guards, the output between pattern guards:
      the output has the bits of (a), pad channels included, its real channels are finite, no guard and no input has changed;
  (c) for B = 3: images 0 and 2 of every activation / image input are NaN throughout, pad channels included: image 1 of the output
      has the bits of (a).  A halo, unit or plane read that crosses into a neighbouring image meets zero padding weights in (a),
      where garbage x 0 = 0 hides it; NaN x 0 = NaN does not.
Every comparison between runs is an equality.  mz_op_final runs with clamp = 0: a clamp built from min / max may swallow a NaN.
TINY_CASES are the same row groups on the smallest images: 1 x 1, a single row, a single column, 2 x 3, and sixteen one-pixel images."""

import ctypes
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from gpu_util import DTYPES, alloc_act, assert_op_close, from_act, last_kernel, pad16, q, stream_ptr, to_act, ulp_of
from oracle import mewzoom_oracle as oracle
from poison_util import Arena
from ultrazoom_amd import _ffi
from ultrazoom_amd.synth import hash_uniform

KNOBS = ("MZ_NO_WIDE", "MZ_NO_FUSE", "MZ_NO_S16", "MZ_NO_FUSE16", "MZ_NO_MIX16B", "MZ_NO_R", "MZ_NO_T", "MZ_NO_R2", "MZ_NO_BLK4",
         "MZ_KPAD_PCT", "MZ_NO_PERSIST", "MZ_PERSIST_WGS")
ALL, LOW = ("f32", "bf16", "f16"), ("bf16", "f16")

# (entry, arguments, environment knobs, dtype, expected mz_debug_last_kernel(); None: the entry's kernel is not a 3x3 / mix family)
CASES = []


def add(entry, args, kernel, dts=LOW, env=None):
    """One row per dtype, and a twin with B = 3 at the same H and W for the NaN-neighbour run.  `kernel`: one name, or one per dtype."""
    twin = (3,) + tuple(args[1:])
    for a in dict.fromkeys((tuple(args), twin)):
        for dt in dts:
            CASES.append((entry, a, dict(env or {}), dt, kernel[dt] if isinstance(kernel, dict) else kernel))


# entry "conv": B, H, W, cin, cout, silu                       "d2s": B, H, W, cin, cout, Hout, Wout (sub-pixel conv + zero border)
# conv3r where the host chooses it: 8 x 48 or 8 x 40 tiles, whichever pads fewer pixels, and only where that is no more than conv3s's
# 8 x 64 / 16 x 32 tiles pad.  (1, 24, 50, 96, 80) and the D2S of 128 -> 4 x 24 channels are conv3s's by that rule (the second because
# its padded 4 x 32 output channels are no 96-channel N tile); (1, 24, 48, 96, 80) and 96 -> 4 x 48 put the same edges on conv3r.
R_SHAPES = {(1, 8, 48, 96, 96, 0): "conv3r",        # one tile
            (2, 13, 37, 128, 96, 1): "conv3r_8x40",  # ragged in both directions
            (1, 24, 50, 96, 80, 1): "conv3s",        # Cout = 80: the N tile's last plane pair does not exist
            (1, 24, 48, 96, 80, 1): "conv3r",
            (3, 23, 117, 96, 96, 1): "conv3r_8x40"}
R_D2S = {(1, 20, 37, 96, 192, 41, 75): "conv3r_8x40",  # targets one larger than 2H x 2W: the zero border
         (1, 16, 48, 128, 96, 33, 97): "conv3s",
         (1, 16, 48, 96, 192, 33, 97): "conv3r"}
RAG_SHAPES = [(2, 13, 37, 48, 192, 1), (1, 27, 200, 48, 80, 1)]                       # Cin = 48 (+ Cout = 80)
T_SHAPES = [(2, 13, 37, 96, 48, 0), (2, 25, 65, 96, 33, 0)]                           # tile larger than the image; Cout = 33
R_FUSED = [(2, 13, 37, 192, 96), (1, 20, 60, 192, 88)]                                # entry "conv_mix": B, H, W, cin, cout
T_FUSED = [(1, 27, 200, 96, 40)]
for s, k in R_SHAPES.items():
    add("conv", s, k)
    add("conv", s, "conv3s", env={"MZ_NO_R": "1"})
for s in RAG_SHAPES:
    add("conv", s, "conv3r_ragged")
for s, k in R_D2S.items():
    add("d2s", s, k)
    add("d2s", s, "conv3s", env={"MZ_NO_R": "1"})
for s in R_FUSED:
    add("conv_mix", s, "conv3r_fused")
    add("conv_mix", s, "conv3s_fused", env={"MZ_NO_R": "1"})
for s in T_SHAPES:
    add("conv", s, "conv3t")
    add("conv", s, "conv3s", env={"MZ_NO_T": "1"})
for s in T_FUSED:
    add("conv_mix", s, "conv3t_fused")
    add("conv_mix", s, "conv3s_fused", env={"MZ_NO_T": "1"})
# persistent 32x32x16 kernel: a shape of test_ops_gpu.PERSIST_CASES (Cin = 16 never fits 32-channel chunks), and Cin = 112
add("conv", (3, 33, 65, 16, 288, 1), "conv3p", dts=ALL, env={"MZ_PERSIST_WGS": "8"})
add("conv", (1, 20, 130, 112, 96, 0), "conv3p", dts=ALL, env={"MZ_PERSIST_WGS": "8"})
for s in [(2, 13, 37, 16, 48, 1), (1, 5, 9, 160, 16, 0), (1, 9, 33, 24, 40, 0)]:      # one workgroup per tile
    add("conv", s, "conv3w", dts=ALL, env={"MZ_NO_PERSIST": "1"})
add("conv_mix", (2, 13, 37, 192, 96), "conv3w_fused", env={"MZ_NO_S16": "1"})          # the per-tile fused kernel
add("conv", (1, 9, 33, 24, 40, 0), "conv_kernel", dts=ALL, env={"MZ_NO_WIDE": "1"})    # the 256-pixel kernel
add("crush", (1, 21, 19, 24, 40), None, dts=ALL)                                       # conv_kernel's 2x2 gather, odd H and W
add("mix", (1, 16, 17, 24), "conv_kernel_mix", dts=ALL)                                # entry "mix": B, H, W, C
add("mix", (2, 11, 29, 384), {"f32": "conv_kernel_mix", "bf16": "mix16", "f16": "mix16"}, dts=ALL)
add("mix", (3, 7, 23, 192), "mix16", env={"MZ_NO_MIX16B": "1"})
add("mix", (3, 7, 23, 192), "mix16b")
add("mix", (3, 7, 23, 192), "mix16b", env={"MZ_PERSIST_WGS": "8"})
for s in [(2, 9, 11, 16), (1, 8, 8, 24)]:
    add("stem", s, None, dts=ALL)                                                      # B, H, W, C
for s in [(2, 9, 11, 16, 2), (1, 16, 24, 32, 8)]:                                      # B, H, W (conv grid), cin, R
    add("final", s, {"f32": "conv3w", "bf16": "conv_kernel", "f16": "conv_kernel"}, dts=ALL)
add("film", (3, 9, 33, 64, 40, 1), "conv3s")                                           # B, H, W, cin, cout, silu

# ---- the lower edge: the same channel counts, knobs and dtypes on the smallest images ------------------------------------------------
# 1 x 1 (a tile of one real pixel inside a halo that is out of range everywhere else), a single row, a single column and 2 x 3, B = 3
# for the NaN-neighbour run; 1 x 1 once more with B = 16: sixteen one-pixel tiles outnumber eight workgroups, a tile list names sixteen
# images and one 32-pixel unit of mix16 spans them all.  Every expected name is the host's choice at that size:
#   - 8 x 40 tiles pad fewer pixels than 8 x 48 ones on every image this small, so the rows of conv3r's 8 x 48 variant run conv3r_8x40;
#   - a 9 x 1 column would take two 8 x 40 tiles, more padding than one 16 x 32 tile of conv3s: the plain conv3r rows (and their D2S)
#     run conv3s there.  The choice of conv3r_ragged, conv3r_fused, conv3t and conv3t_fused does not depend on H and W;
#   - Cin = 112 reaches conv3p only where the tiles outnumber the eight workgroups (B = 16); the B = 3 rows run conv3w.
TINY = [(3, 1, 1), (16, 1, 1), (3, 1, 9), (3, 9, 1), (3, 2, 3)]
COLUMN = (3, 9, 1)


def add_tiny(entry, rest, kernel, dts=LOW, env=None, other=None, geos=TINY, tail=lambda H, W: ()):
    """One row per geometry and dtype (no twin: B = 3 is in the list).  `other`: geometry -> the family chosen there instead."""
    for g in geos:
        k = (other or {}).get(g, kernel)
        for dt in dts:
            CASES.append((entry, g + tuple(rest) + tuple(tail(g[1], g[2])), dict(env or {}), dt, k[dt] if isinstance(k, dict) else k))


N_TINY_START = len(CASES)
add_tiny("conv", (96, 96, 0), "conv3r_8x40", other={COLUMN: "conv3s"})
add_tiny("conv", (96, 96, 0), "conv3s", env={"MZ_NO_R": "1"})
add_tiny("conv", (128, 96, 1), "conv3r_8x40", other={COLUMN: "conv3s"})
add_tiny("conv", (48, 192, 1), "conv3r_ragged")
add_tiny("d2s", (96, 192), "conv3r_8x40", other={COLUMN: "conv3s"}, tail=lambda H, W: (2 * H, 2 * W))
add_tiny("d2s", (96, 192), "conv3r_8x40", other={COLUMN: "conv3s"}, tail=lambda H, W: (2 * H + 1, 2 * W + 1))  # 1 x 1 -> 3 x 3
add_tiny("d2s", (96, 192), "conv3s", env={"MZ_NO_R": "1"}, tail=lambda H, W: (2 * H + 1, 2 * W + 1))
add_tiny("conv_mix", (192, 96), "conv3r_fused")
add_tiny("conv_mix", (192, 96), "conv3s_fused", env={"MZ_NO_R": "1"})
add_tiny("conv", (96, 48, 0), "conv3t")
add_tiny("conv", (96, 48, 0), "conv3s", env={"MZ_NO_T": "1"})
add_tiny("conv_mix", (96, 40), "conv3t_fused")
add_tiny("conv_mix", (96, 40), "conv3s_fused", env={"MZ_NO_T": "1"})
add_tiny("conv", (16, 288, 1), "conv3p", dts=ALL, env={"MZ_PERSIST_WGS": "8"})
add_tiny("conv", (112, 96, 0), "conv3w", dts=ALL, env={"MZ_PERSIST_WGS": "8"}, other={(16, 1, 1): "conv3p"})
add_tiny("conv", (16, 48, 1), "conv3w", dts=ALL, env={"MZ_NO_PERSIST": "1"})
add_tiny("conv_mix", (192, 96), "conv3w_fused", env={"MZ_NO_S16": "1"})
add_tiny("conv", (24, 40, 0), "conv_kernel", dts=ALL, env={"MZ_NO_WIDE": "1"})
add_tiny("crush", (24, 40), None, dts=ALL, geos=[(3, 2, 2), (3, 3, 3), (3, 2, 9)])      # floors land on 1 x 1 (and 1 x 4)
add_tiny("mix", (24,), "conv_kernel_mix", dts=ALL)
add_tiny("mix", (384,), {"f32": "conv_kernel_mix", "bf16": "mix16", "f16": "mix16"}, dts=ALL)
add_tiny("mix", (192,), "mix16", env={"MZ_NO_MIX16B": "1"})
add_tiny("mix", (192,), "mix16b")
add_tiny("mix", (192,), "mix16b", env={"MZ_PERSIST_WGS": "8"})
add_tiny("stem", (16,), None, dts=ALL, geos=[(3, 1, 1), (3, 2, 3)])
# the head at the model's own minimum (an 8 x 8 conv grid at R = 2), and a 4 x 4 grid at R = 8: the skip image is 1 x 1, every bicubic
# tap clamps to that one pixel
add_tiny("final", (16, 2), {"f32": "conv3w", "bf16": "conv_kernel", "f16": "conv_kernel"}, dts=ALL, geos=[(3, 8, 8)])
add_tiny("final", (32, 8), {"f32": "conv3w", "bf16": "conv_kernel", "f16": "conv_kernel"}, dts=ALL, geos=[(3, 4, 4)])
add_tiny("film", (64, 40, 1), "conv3s", geos=[(3, 1, 1), (3, 2, 3)])
TINY_CASES = CASES[N_TINY_START:]

# the family a row is there for, where the library does not report one (conv_kernel in its 2x2 gather mode)
FAMILY_OF_UNREPORTED = {"crush": "conv_kernel"}


def case_id(case):
    entry, args, env, dt, _ = case
    return "-".join([entry, "x".join(str(v) for v in args), dt] + [f"{k[3:]}={v}" for k, v in env.items()])


def test_the_case_table_names_every_kernel_family():
    """Needs no GPU: every literal kernel_name() (mz_select.h) can return is the expected kernel of some row, so that a family added
    later cannot be forgotten here."""
    src = (Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc" / "mz_select.h").read_text()
    body = re.search(r"inline const char\* kernel_name\(const KernelChoice& ch\) \{(.*?)\n\}\n", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)  # (a comment quotes names, too)
    names = set(re.findall(r'"([a-z0-9_]+)"', body))
    assert len(names) >= 15 and {"conv3r", "conv3t_fused", "mix16b", "conv_kernel_mix"} <= names, names
    covered = {c[4] for c in CASES if c[4]} | {FAMILY_OF_UNREPORTED[c[0]] for c in CASES if c[0] in FAMILY_OF_UNREPORTED}
    assert names <= covered, f"no row of CASES runs {sorted(names - covered)}"
    assert all(c[3] in DTYPES for c in CASES)
    assert len({case_id(c) for c in CASES}) == len(CASES)


SELECT_OP = {"conv": None, "d2s": 2, "conv_mix": 6, "mix": 7, "final": 3, "film": 5}


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in SELECT_OP], ids=case_id)
def test_the_expected_kernels_are_the_host_s_choice(case, monkeypatch):
    """Needs no GPU: the expected name of every row is what choose_conv3 / choose_mix choose on an MI355X (256 CUs)."""
    entry, args, env, dt, kernel = case
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = _ffi.lib()
    lib.mz_debug_select.restype = ctypes.c_char_p
    B, H, W = args[:3]
    if entry == "mix":
        op, cin, cout = 7, 2 * args[3], args[3]
    elif entry == "final":
        op, cin, cout = 3, args[3], 12
    else:
        cin, cout = args[3:5]
        op = SELECT_OP[entry] if entry != "conv" else (0 if args[5] else 1)
    got = lib.mz_debug_select(_ffi.dtype_code(DTYPES[dt]), op, cin, cout, B, H, W, 256)
    assert got is not None and got.decode() == kernel, (got, kernel)


def rnd(shape, seed, scale=1.0):
    n = 1
    for s in shape:
        n *= s
    return torch.from_numpy(((2.0 * hash_uniform(n, seed) - 1.0) * scale).reshape(shape))


def wrnd(shape, seed):
    fan_in = shape[1] * shape[2] * shape[3]
    return rnd(shape, seed, (3.0 / fan_in) ** 0.5 * 1.7)


class Op:
    """One operator call: its device tensors by argument name, which of them hold one entry per image, its output and its oracle."""

    def __init__(self, entry, args, dt):
        self.entry, self.args, self.dt = entry, args, dt
        dtype = self.dtype = DTYPES[dt]
        B, H, W = args[:3]
        self.alpha = 0.0
        self.tol = None  # element-wise tolerance where it is not gpu_util's one-operator tolerance
        dev_w = lambda w: w.to("cuda", torch.float32).contiguous()
        if entry in ("conv", "film"):
            _, _, _, cin, cout, silu = args
            x, w = q(rnd((B, cin, H, W), 1), dtype), q(wrnd((cout, cin, 3, 3), 2), dtype)
            self.t, self.batched = {"in0": to_act(x, dtype), "w": dev_w(w)}, ["in0"]
            self.C, self.out_shape = cout, alloc_act(B, cout, H, W, dtype).shape
            if entry == "film":
                gamma, beta = 1.0 + 0.5 * rnd((B, cout), 43), 0.3 * rnd((B, cout), 44)
                self.t.update(gamma=dev_w(gamma), beta=dev_w(beta))
                self.want = oracle.film_conv(x, w, gamma.float(), beta.float(), bool(silu))
            else:
                self.want = F.conv2d(x, w, padding=1)
                if silu:
                    self.want = F.silu(self.want)
        elif entry == "d2s":
            _, _, _, cin, cout, Hout, Wout = args
            x, w = q(rnd((B, cin, H, W), 3), dtype), q(wrnd((cout, cin, 3, 3), 4), dtype)
            self.t, self.batched = {"in0": to_act(x, dtype), "w": dev_w(w)}, ["in0"]
            self.C, self.out_shape = cout // 4, alloc_act(B, cout // 4, Hout, Wout, dtype).shape
            self.want = oracle.fit_to(oracle.subpixel_conv(x, w), (Hout, Wout))
        elif entry == "crush":
            _, _, _, cin, cout = args
            x, w = q(rnd((B, cin, H, W), 5), dtype), q(wrnd((cout, cin, 2, 2), 6), dtype)
            self.t, self.batched = {"in0": to_act(x, dtype), "w": dev_w(w)}, ["in0"]
            self.C, self.out_shape = cout, alloc_act(B, cout, H // 2, W // 2, dtype).shape
            self.want = F.conv2d(x, w, stride=2)
        elif entry == "mix":
            c = args[3]
            x, z, w = q(rnd((B, c, H, W), 7), dtype), q(rnd((B, c, H, W), 8), dtype), q(wrnd((c, 2 * c, 1, 1), 9), dtype)
            self.alpha = 0.37
            self.t, self.batched = {"in0": to_act(x, dtype), "in1": to_act(z, dtype), "w": dev_w(w)}, ["in0", "in1"]
            self.C, self.out_shape = c, alloc_act(B, c, H, W, dtype).shape
            self.want = oracle.residual_mix(x, z, w, torch.tensor(self.alpha))
        elif entry == "conv_mix":
            _, _, _, cin, cout = args
            hid, x = q(rnd((B, cin, H, W), 41), dtype), q(rnd((B, cout, H, W), 42), dtype)
            w2, wmix = q(wrnd((cout, cin, 3, 3), 43), dtype), q(rnd((cout, 2 * cout, 1, 1), 44, (3.0 / (2 * cout)) ** 0.5 * 1.7), dtype)
            self.alpha = 0.3
            self.t, self.batched = {"hid": to_act(hid, dtype), "x": to_act(x, dtype), "w2": dev_w(w2), "wmix": dev_w(wmix)}, ["hid", "x"]
            self.C, self.out_shape = cout, alloc_act(B, cout, H, W, dtype).shape
            # the kernel rounds z to the storage type before the gate GEMM and the blend, as the unfused path stores it: one rounding
            # of the output plus one rounding step of z where its fp32 sum sits on a boundary (tests/test_conv3r_gpu.py)
            z = q(F.conv2d(hid, w2, padding=1), dtype)
            self.want = oracle.residual_mix(x, z, wmix, torch.tensor(self.alpha))
            self.tol = ulp_of(self.want, dt) + ulp_of(z, dt) + 1e-5
        elif entry == "stem":
            c = args[3]
            x, w, b = q(rnd((B, 3, H, W), 10).abs(), dtype), rnd((c, 3, 1, 1), 11), rnd((c,), 12, 0.1)
            self.t, self.batched = {"x": x.to("cuda", dtype).contiguous(), "w": dev_w(w), "b": dev_w(b)}, ["x"]
            self.C, self.out_shape = c, alloc_act(B, c, H, W, dtype).shape
            self.want = F.conv2d(x, w, b)
        elif entry == "final":
            _, _, _, cin, R = args
            Hi, Wi = 2 * H // R, 2 * W // R
            assert Hi * R == 2 * H and Wi * R == 2 * W
            feat, img = q(rnd((B, cin, H, W), 13), dtype), q(rnd((B, 3, Hi, Wi), 14).abs(), dtype)
            w = q(wrnd((12, cin, 3, 3), 15) * 0.5, dtype)
            self.t = {"feat": to_act(feat, dtype), "img": img.to("cuda", dtype).contiguous(), "w": dev_w(w)}
            self.batched = ["feat", "img"]
            self.C, self.out_shape = None, (B, 3, 2 * H, 2 * W)  # a dense NCHW image
            self.want = oracle.bicubic_upsample(img, R) + oracle.subpixel_conv(feat, w)
        else:
            raise ValueError(entry)

    @classmethod
    def call_only(cls, entry, args, dt, alpha=0.0):
        """An Op that has no tensors or oracle of its own: run() alone, on tensors the caller brings (tests/test_exact_gpu.py,
        tests/test_large_offsets_gpu.py).  Sets exactly what run() reads."""
        op = cls.__new__(cls)
        op.entry, op.args, op.dt, op.dtype, op.alpha = entry, tuple(args), dt, DTYPES[dt], alpha
        return op

    def real(self, out):
        """The output's real channels as float32 [B, C, H, W] on the CPU."""
        return out.float().cpu() if self.C is None else from_act(out, self.C)

    def run(self, t, out):
        lib, d, p, s = _ffi.lib(), _ffi.dtype_code(self.dtype), (lambda v: ctypes.c_void_p(v.data_ptr())), ctypes.c_void_p(stream_ptr())
        e, a = self.entry, self.args
        B, H, W = a[:3]
        if e in ("conv", "d2s", "crush", "mix"):
            kind = {"conv": 0, "d2s": 1, "crush": 2, "mix": 3}[e]
            cin, cout = (2 * a[3], a[3]) if e == "mix" else a[3:5]
            Hout, Wout = a[5:7] if e == "d2s" else (0, 0)
            rc = lib.mz_op_conv(d, kind, p(t["in0"]), p(t["in1"]) if e == "mix" else None, p(t["w"]), ctypes.c_float(self.alpha), p(out),
                                B, H, W, cin, cout, Hout, Wout, a[5] if e == "conv" else 0, s)
        elif e == "conv_mix":
            rc = lib.mz_op_conv_mix(d, p(t["hid"]), p(t["x"]), p(t["w2"]), p(t["wmix"]), ctypes.c_float(self.alpha), p(out), B, H, W, a[3], a[4], s)
        elif e == "film":
            rc = lib.mz_op_conv_film(d, p(t["in0"]), p(t["w"]), p(t["gamma"]), p(t["beta"]), p(out), B, H, W, a[3], a[4], a[5], s)
        elif e == "stem":
            rc = lib.mz_op_stem(d, p(t["x"]), p(t["w"]), p(t["b"]), p(out), B, H, W, a[3], s)
        else:
            rc = lib.mz_op_final(d, p(t["feat"]), p(t["img"]), p(t["w"]), p(out), B, H, W, a[3], a[4], 0, s)
        _ffi.check(rc)
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_poisoned_surroundings(case, monkeypatch):
    entry, args, env, dt, kernel = case
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    op = Op(entry, args, dt)
    # (a) ordinary tensors
    plain = torch.full(op.out_shape, 7.0, dtype=op.dtype, device="cuda")
    op.run(op.t, plain)
    if kernel is not None:
        assert last_kernel() == kernel, (last_kernel(), kernel)
    got = op.real(plain)
    if op.tol is None:
        assert_op_close(got, op.want, dt, entry)
    else:
        ex = ((got - op.want).abs() / op.tol).max().item()
        assert ex <= 1.0, f"{entry} {dt}: {ex:.2f} x (ulp(out) + ulp(z) + 1e-5)"
    if op.C is not None and pad16(op.C) > op.C:
        B, P, H, W, ppu = plain.shape
        assert bool((plain.permute(0, 1, 4, 2, 3).reshape(B, P * ppu, H, W)[:, op.C:] == 0).all()), "pad channels must be written as zeros"
    # (b) every pointer inside an arena; the output starts from another value than in (a): an element nobody writes differs
    arena = Arena("cuda")
    tb = {k: arena.input(v, name=k) for k, v in op.t.items()}
    out = arena.output(op.out_shape, op.dtype, fill=-3.0, name="out")
    op.run(tb, out)
    if kernel is not None:
        assert last_kernel() == kernel, (last_kernel(), kernel)
    arena.check()
    assert bool(torch.isfinite(op.real(out)).all()), "NaN guards around the inputs reached the output"
    assert torch.equal(out, plain), "the result depends on what surrounds the tensors"
    # (c) NaN neighbours
    if args[0] == 3:
        tc = dict(op.t)
        for k in op.batched:
            v = op.t[k].clone()
            v[0] = float("nan")
            v[2] = float("nan")
            tc[k] = v
        lone = torch.full(op.out_shape, -3.0, dtype=op.dtype, device="cuda")
        op.run(tc, lone)
        assert bool(torch.isfinite(lone[1].float()).all()), "image 1 read a NaN of its neighbours"
        assert torch.equal(lone[1], plain[1]), "image 1 depends on its neighbours"
        assert bool(torch.isnan(op.real(lone)[0::2]).any()), "the NaN images themselves must not come out clean"
