"""The family table of the operator tests: every operator entry, how its call is written, and the rows that pin every kernel family.
Pure data, no GPU.  A new kernel family is registered HERE: its rows in CASES (and TINY_CASES), with the knobs that pin it and the name
mz_debug_last_kernel() reports; tests/op_util.py runs the rows, tests/exact_util.py and tests/large_util.py build their tables on them.
A new ENTRY gets its argument names in ARGS; what it is (inputs and their roles, output, reference) is stated once in tests/op_ref.py."""

from types import SimpleNamespace

# every knob read_knobs() (mz_plan.h) reads; tests/test_layout.py holds the two to each other
KNOBS = ("MZ_NO_WIDE", "MZ_NO_FUSE", "MZ_NO_S16", "MZ_NO_FUSE16", "MZ_NO_MIX16B", "MZ_NO_R", "MZ_NO_T", "MZ_NO_R2", "MZ_NO_BLK4",
         "MZ_KPAD_PCT", "MZ_NO_PERSIST", "MZ_PERSIST_WGS")
ALL, LOW = ("f32", "bf16", "f16"), ("bf16", "f16")

# An operator call is (entry, positional arguments).  H, W: the conv grid (crush: its input; final: 2 H x 2 W is the image that comes
# out, at R times the skip image).  d2s: sub-pixel conv + zero border up to Hout x Wout.  clamp may be left out (0).
ARGS = {"conv": ("B", "H", "W", "cin", "cout", "silu"),
        "film": ("B", "H", "W", "cin", "cout", "silu"),
        "d2s": ("B", "H", "W", "cin", "cout", "Hout", "Wout"),
        "crush": ("B", "H", "W", "cin", "cout"),
        "mix": ("B", "H", "W", "C"),
        "conv_mix": ("B", "H", "W", "cin", "cout"),
        "stem": ("B", "H", "W", "C"),
        "final": ("B", "H", "W", "cin", "R", "clamp")}
# mz_debug_select's op of an entry ("conv": 0 with SiLU -- conv1 --, 1 without); the other entries choose no 3x3 / mix family
SELECT_OP = {"d2s": 2, "final": 3, "film": 5, "conv_mix": 6, "mix": 7}
# the family a row is there for, where the library does not report one (conv_kernel in its 2x2 gather mode)
FAMILY_OF_UNREPORTED = {"crush": "conv_kernel"}


def fields(entry, args):
    """The arguments of one call by name."""
    names = ARGS[entry]
    assert len(names) - (names[-1] == "clamp") <= len(args) <= len(names), (entry, args)
    return SimpleNamespace(**dict(zip(names, tuple(args) + (0,))))


def select_args(entry, args, silu=None):
    """(op, cin, cout) of mz_debug_select; None where the entry chooses no 3x3 / mix family.  `silu` overrides a conv's own."""
    f = fields(entry, args)
    if entry == "conv":
        return (0 if (f.silu if silu is None else silu) else 1, f.cin, f.cout)
    if entry == "mix":
        return (7, 2 * f.C, f.C)
    if entry == "final":
        return (3, f.cin, 12)
    return (SELECT_OP[entry], f.cin, f.cout) if entry in SELECT_OP else None


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


def case_id(case):
    entry, args, env, dt, _ = case
    return "-".join([entry, "x".join(str(v) for v in args), dt] + [f"{k[3:]}={v}" for k, v in env.items()])
