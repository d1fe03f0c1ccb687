"""What every operator entry IS, stated once (needs no GPU): its inputs by name with their logical shapes and roles, the real channels
and logical shape of its output, its reference, its sums of absolute products and the pieces of the two mixes.  Everything is computed
in the dtype of the tensors handed in: float32 for tests/op_util.Op, float64 for the exact tables (tests/exact_util.py,
tests/range_util.py), which only DRAW their tensors and leave the rest to this table; tests/op_util.py uploads by the roles.  A new
entry gets its argument names in op_cases.ARGS, its call in op_util.run_entry and its statement HERE."""

from collections import namedtuple
from functools import cached_property

import torch
import torch.nn.functional as F

from op_cases import fields
from oracle import mewzoom_oracle as oracle

# roles of an input: a plane-major activation tensor, a dense NCHW image (both in the storage type, one entry per image), or a
# parameter, which travels as float32
ACT, IMG, PAR = "activation", "image", "parameter"
MIXES = ("mix", "conv_mix")

# With `a` the call's arguments by name (op_cases.fields) and `t` its inputs as logical tensors by name:
#   inputs(a)              {name: (logical shape, role)} in the order of the call
#   output(a)              (real channels C, None for a dense image; logical [B, C, Hout, Wout])
#   reference(a, t, silu)  the result; None for the mixes, whose blend stays with the consumer (Mix)
#   sums(t)                largest sum of absolute products of each quantity accumulated before a mix ("conv", "film", "stem")
Entry = namedtuple("Entry", "inputs output reference sums")


def abs_sum(x, w, **kw):
    return F.conv2d(x.abs(), w.abs(), **kw).max().item()


def _act(a, c):
    return (a.B, c, a.H, a.W), ACT


def _conv_inputs(a, k=3):
    return {"in0": _act(a, a.cin), "w": ((a.cout, a.cin, k, k), PAR)}


def _same(a):
    return a.cout, (a.B, a.cout, a.H, a.W)


def _conv(t, silu=False, **kw):
    y = F.conv2d(t["in0"], t["w"], **kw)
    return F.silu(y) if silu else y


def _conv_sum(t):
    return {"conv": abs_sum(t["in0"], t["w"], padding=1)}


def _film_sum(t):
    per = lambda v: v.abs()[:, :, None, None]
    return {**_conv_sum(t), "film": (F.conv2d(t["in0"].abs(), t["w"].abs(), padding=1) * per(t["gamma"]) + per(t["beta"])).max().item()}


ENTRIES = {
    "conv": Entry(_conv_inputs, _same, lambda a, t, silu: _conv(t, silu, padding=1), _conv_sum),
    "film": Entry(lambda a: {**_conv_inputs(a), "gamma": ((a.B, a.cout), PAR), "beta": ((a.B, a.cout), PAR)}, _same,
                  lambda a, t, silu: oracle.film_conv(t["in0"], t["w"], t["gamma"], t["beta"], bool(silu)), _film_sum),
    "d2s": Entry(_conv_inputs, lambda a: (a.cout // 4, (a.B, a.cout // 4, a.Hout, a.Wout)),
                 lambda a, t, silu: oracle.fit_to(oracle.subpixel_conv(t["in0"], t["w"]), (a.Hout, a.Wout)), _conv_sum),
    "crush": Entry(lambda a: _conv_inputs(a, 2), lambda a: (a.cout, (a.B, a.cout, a.H // 2, a.W // 2)),
                   lambda a, t, silu: _conv(t, stride=2), lambda t: {"conv": abs_sum(t["in0"], t["w"], stride=2)}),
    "mix": Entry(lambda a: {"in0": _act(a, a.C), "in1": _act(a, a.C), "w": ((a.C, 2 * a.C, 1, 1), PAR)},
                 lambda a: (a.C, (a.B, a.C, a.H, a.W)), None, lambda t: {}),
    "conv_mix": Entry(lambda a: {"hid": _act(a, a.cin), "x": _act(a, a.cout), "w2": ((a.cout, a.cin, 3, 3), PAR),
                                 "wmix": ((a.cout, 2 * a.cout, 1, 1), PAR)},
                      _same, None, lambda t: {"conv": abs_sum(t["hid"], t["w2"], padding=1)}),
    "stem": Entry(lambda a: {"x": ((a.B, 3, a.H, a.W), IMG), "w": ((a.C, 3, 1, 1), PAR), "b": ((a.C,), PAR)},
                  lambda a: (a.C, (a.B, a.C, a.H, a.W)), lambda a, t, silu: F.conv2d(t["x"], t["w"], t["b"]),
                  lambda t: {"stem": F.conv2d(t["x"], t["w"].abs(), t["b"].abs()).max().item()}),  # the image is not negative
    # H x W is the conv grid: 2 H x 2 W comes out, at R times the skip image
    "final": Entry(lambda a: {"feat": _act(a, a.cin), "img": ((a.B, 3, 2 * a.H // a.R, 2 * a.W // a.R), IMG), "w": ((12, a.cin, 3, 3), PAR)},
                   lambda a: (None, (a.B, 3, 2 * a.H, 2 * a.W)),
                   lambda a, t, silu: oracle.bicubic_upsample(t["img"], a.R) + oracle.subpixel_conv(t["feat"], t["w"]),
                   lambda t: {"conv": abs_sum(t["feat"], t["w"], padding=1)}),
}


def inputs(entry, args):
    return ENTRIES[entry].inputs(fields(entry, args))


def shapes(entry, args):
    """{input name: logical shape}"""
    return {k: shape for k, (shape, _) in inputs(entry, args).items()}


def check_shapes(entry, args, t):
    """`t` holds the entry's inputs and nothing else, each of its logical shape."""
    got, want = {k: tuple(v.shape) for k, v in t.items()}, shapes(entry, args)
    assert got == want, (entry, args, got, want)


def output(entry, args):
    return ENTRIES[entry].output(fields(entry, args))


def reference(entry, args, t, silu=None):
    """`silu` overrides the call's own (False: the result before the SiLU)."""
    a = fields(entry, args)
    return ENTRIES[entry].reference(a, t, getattr(a, "silu", 0) if silu is None else silu)


def abs_sums(entry, t):
    return ENTRIES[entry].sums(t)


class Mix:
    """The pieces of a residual mix that every consumer needs: x, z (conv_mix: the 3x3 result `z_raw` passed through `round_z`, the
    rounding to the storage type that the kernel applies before the gate GEMM and the blend, as the unfused path stores z), [x ; z],
    the gate and the mix's own sums of absolute products.  The blend itself is the consumer's."""

    def __init__(self, entry, t, round_z=lambda z: z):
        if entry == "mix":
            self.x, self.z_raw, self.w = t["in0"], t["in1"], t["w"]
            self.z = self.z_raw
        else:
            self.x, self.z_raw, self.w = t["x"], F.conv2d(t["hid"], t["w2"], padding=1), t["wmix"]
            self.z = round_z(self.z_raw)

    @cached_property
    def xz(self):
        return torch.cat([self.x, self.z], dim=1)

    @cached_property
    def gate(self):
        return F.conv2d(self.xz, self.w)

    def abs_sums(self):
        return {"gate": abs_sum(self.xz, self.w), "blend": (self.x.abs() + self.z.abs()).max().item()}
