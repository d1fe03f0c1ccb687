"""The runner of the operator tests: knobs, seeded data, the ONE call of each mz_op_* entry (run_entry), the tensors and oracle of a row
of tests/op_cases.py (Op), and the host's choice read without a GPU (selected).  A new entry gets its names in op_cases.ARGS, its call in
run_entry and its tensors in Op."""

import ctypes
import re
from pathlib import Path

import torch
import torch.nn.functional as F

from gpu_util import DTYPES, alloc_act, from_act, q, stream_ptr, to_act, ulp_of
from op_cases import KNOBS, fields, select_args
from oracle import mewzoom_oracle as oracle
from ultrazoom_amd import _ffi
from ultrazoom_amd.synth import hash_uniform

CSRC = Path(__file__).resolve().parent.parent / "ultrazoom_amd" / "csrc"


def set_knobs(monkeypatch, env=None, wgs=None):
    """Every knob out of the environment, then `env`'s, then MZ_PERSIST_WGS = wgs (0 / None / "": left unset)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if wgs:
        monkeypatch.setenv("MZ_PERSIST_WGS", str(wgs))


def rnd(shape, seed, scale=1.0):
    n = 1
    for s in shape:
        n *= s
    return torch.from_numpy(((2.0 * hash_uniform(n, seed) - 1.0) * scale).reshape(shape))


def wrnd(shape, seed):
    fan_in = shape[1] * shape[2] * shape[3]
    return rnd(shape, seed, (3.0 / fan_in) ** 0.5 * 1.7)


def dev_w(w):
    """Weights travel as float32."""
    return w.to("cuda", torch.float32).contiguous()


KIND = {"conv": 0, "d2s": 1, "crush": 2, "mix": 3}  # mz_op_conv's roles


def run_entry(entry, args, dt, tensors, out, alpha=0.0, check=True):
    """One call of the entry on device tensors by argument name, then a synchronize.  dt: "f32" / "bf16" / "f16" or the torch dtype.
    Returns the entry's code (check = False: also where it refuses).  mz_op_final's clamp is 0 unless `args` carries one."""
    lib, d, s = _ffi.lib(), _ffi.dtype_code(DTYPES.get(dt, dt)), ctypes.c_void_p(stream_ptr())
    p, o, f = (lambda name: ctypes.c_void_p(tensors[name].data_ptr())), ctypes.c_void_p(out.data_ptr()), fields(entry, args)
    if entry in KIND:
        cin, cout = (2 * f.C, f.C) if entry == "mix" else (f.cin, f.cout)
        rc = lib.mz_op_conv(d, KIND[entry], p("in0"), p("in1") if entry == "mix" else None, p("w"), ctypes.c_float(alpha), o,
                            f.B, f.H, f.W, cin, cout, getattr(f, "Hout", 0), getattr(f, "Wout", 0), getattr(f, "silu", 0), s)
    elif entry == "conv_mix":
        rc = lib.mz_op_conv_mix(d, p("hid"), p("x"), p("w2"), p("wmix"), ctypes.c_float(alpha), o, f.B, f.H, f.W, f.cin, f.cout, s)
    elif entry == "film":
        rc = lib.mz_op_conv_film(d, p("in0"), p("w"), p("gamma"), p("beta"), o, f.B, f.H, f.W, f.cin, f.cout, f.silu, s)
    elif entry == "stem":
        rc = lib.mz_op_stem(d, p("x"), p("w"), p("b"), o, f.B, f.H, f.W, f.C, s)
    else:
        rc = lib.mz_op_final(d, p("feat"), p("img"), p("w"), o, f.B, f.H, f.W, f.cin, f.R, f.clamp, s)
    if check:
        _ffi.check(rc)
    torch.cuda.synchronize()
    return rc


def op_conv(dtype, kind, in0, in1, w, alpha, out, B, H, W, cin, cout, Hout=0, Wout=0, silu=0):
    """run_entry for mz_op_conv's role `kind`, weights from the host."""
    entry = list(KIND)[kind]
    args = {"conv": (B, H, W, cin, cout, silu), "d2s": (B, H, W, cin, cout, Hout, Wout), "crush": (B, H, W, cin, cout), "mix": (B, H, W, cout)}
    run_entry(entry, args[entry], dtype, {"in0": in0, "in1": in1, "w": dev_w(w)}, out, alpha)


def op_conv_mix(dtype, hid, x, w2, wmix, alpha, out, B, H, W, cin, cout):
    run_entry("conv_mix", (B, H, W, cin, cout), dtype, {"hid": hid, "x": x, "w2": dev_w(w2), "wmix": dev_w(wmix)}, out, alpha)


class Op:
    """One operator call: its device tensors by argument name, which of them hold one entry per image, its output and its oracle."""

    def __init__(self, entry, args, dt):
        self.entry, self.args, self.dt = entry, args, dt
        dtype = self.dtype = DTYPES[dt]
        a = fields(entry, args)
        B, H, W = a.B, a.H, a.W
        self.alpha = 0.0
        self.tol = None  # element-wise tolerance where it is not gpu_util's one-operator tolerance
        if entry in ("conv", "film"):
            x, w = q(rnd((B, a.cin, H, W), 1), dtype), q(wrnd((a.cout, a.cin, 3, 3), 2), dtype)
            self.t, self.batched = {"in0": to_act(x, dtype), "w": dev_w(w)}, ["in0"]
            self.C, self.out_shape = a.cout, alloc_act(B, a.cout, H, W, dtype).shape
            if entry == "film":
                gamma, beta = 1.0 + 0.5 * rnd((B, a.cout), 43), 0.3 * rnd((B, a.cout), 44)
                self.t.update(gamma=dev_w(gamma), beta=dev_w(beta))
                self.want = oracle.film_conv(x, w, gamma.float(), beta.float(), bool(a.silu))
            else:
                self.want = F.conv2d(x, w, padding=1)
                if a.silu:
                    self.want = F.silu(self.want)
        elif entry == "d2s":
            x, w = q(rnd((B, a.cin, H, W), 3), dtype), q(wrnd((a.cout, a.cin, 3, 3), 4), dtype)
            self.t, self.batched = {"in0": to_act(x, dtype), "w": dev_w(w)}, ["in0"]
            self.C, self.out_shape = a.cout // 4, alloc_act(B, a.cout // 4, a.Hout, a.Wout, dtype).shape
            self.want = oracle.fit_to(oracle.subpixel_conv(x, w), (a.Hout, a.Wout))
        elif entry == "crush":
            x, w = q(rnd((B, a.cin, H, W), 5), dtype), q(wrnd((a.cout, a.cin, 2, 2), 6), dtype)
            self.t, self.batched = {"in0": to_act(x, dtype), "w": dev_w(w)}, ["in0"]
            self.C, self.out_shape = a.cout, alloc_act(B, a.cout, H // 2, W // 2, dtype).shape
            self.want = F.conv2d(x, w, stride=2)
        elif entry == "mix":
            c = a.C
            x, z, w = q(rnd((B, c, H, W), 7), dtype), q(rnd((B, c, H, W), 8), dtype), q(wrnd((c, 2 * c, 1, 1), 9), dtype)
            self.alpha = 0.37
            self.t, self.batched = {"in0": to_act(x, dtype), "in1": to_act(z, dtype), "w": dev_w(w)}, ["in0", "in1"]
            self.C, self.out_shape = c, alloc_act(B, c, H, W, dtype).shape
            self.want = oracle.residual_mix(x, z, w, torch.tensor(self.alpha))
        elif entry == "conv_mix":
            cin, cout = a.cin, a.cout
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
            c = a.C
            x, w, b = q(rnd((B, 3, H, W), 10).abs(), dtype), rnd((c, 3, 1, 1), 11), rnd((c,), 12, 0.1)
            self.t, self.batched = {"x": x.to("cuda", dtype).contiguous(), "w": dev_w(w), "b": dev_w(b)}, ["x"]
            self.C, self.out_shape = c, alloc_act(B, c, H, W, dtype).shape
            self.want = F.conv2d(x, w, b)
        elif entry == "final":
            Hi, Wi = 2 * H // a.R, 2 * W // a.R
            assert Hi * a.R == 2 * H and Wi * a.R == 2 * W
            feat, img = q(rnd((B, a.cin, H, W), 13), dtype), q(rnd((B, 3, Hi, Wi), 14).abs(), dtype)
            w = q(wrnd((12, a.cin, 3, 3), 15) * 0.5, dtype)
            self.t = {"feat": to_act(feat, dtype), "img": img.to("cuda", dtype).contiguous(), "w": dev_w(w)}
            self.batched = ["feat", "img"]
            self.C, self.out_shape = None, (B, 3, 2 * H, 2 * W)  # a dense NCHW image
            self.want = oracle.bicubic_upsample(img, a.R) + oracle.subpixel_conv(feat, w)
        else:
            raise ValueError(entry)

    def real(self, out):
        """The output's real channels as float32 [B, C, H, W] on the CPU."""
        return out.float().cpu() if self.C is None else from_act(out, self.C)

    def run(self, t, out):
        run_entry(self.entry, self.args, self.dt, t, out, self.alpha)


def select_op(dtype_code, op, cin, cout, B, H, W, cus=256):
    """mz_debug_select: the family the host chooses on `cus` CUs (256: an MI355X), None where it refuses.  Needs no GPU."""
    lib = _ffi.lib()
    lib.mz_debug_select.restype = ctypes.c_char_p
    got = lib.mz_debug_select(dtype_code, op, cin, cout, B, H, W, cus)
    return None if got is None else got.decode()


def selected(entry, args, dt, silu=None, cus=256):
    """select_op for an entry's call (op_cases.select_args)."""
    return select_op(_ffi.dtype_code(DTYPES.get(dt, dt)), *select_args(entry, args, silu), *args[:3], cus)


def _body(header, signature):
    """The body of the one function of ultrazoom_amd/csrc/<header> that starts with `signature`, comments removed (they quote names, too)."""
    body = re.search(re.escape(signature) + r" \{(.*?)\n\}\n", (CSRC / header).read_text(), re.S).group(1)
    return re.sub(r"//[^\n]*", "", body)


def kernel_names():
    """Every literal kernel_name() (mz_select.h) can return."""
    names = set(re.findall(r'"([a-z0-9_]+)"', _body("mz_select.h", "inline const char* kernel_name(const KernelChoice& ch)")))
    assert len(names) >= 15 and {"conv3r", "conv3t_fused", "mix16b", "conv_kernel_mix"} <= names, names
    return names


def knob_names():
    """Every name read_knobs() (mz_plan.h) passes to getenv."""
    return set(re.findall(r'getenv\("(\w+)"\)', _body("mz_plan.h", "inline Knobs read_knobs()")))
