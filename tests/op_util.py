"""The runner of the operator tests: knobs, seeded data, the ONE call of each mz_op_* entry (run_entry), the ONE way an entry's tensors
reach the GPU and its output comes back (upload, alloc_out, real, launch: by the roles of tests/op_ref.py), the ONE check of a row of the
exact tables (check_rounded_once), the seeded data and oracle of a row of tests/op_cases.py (Op), and the host's choice read without a
GPU (selected).  A new entry gets its names in op_cases.ARGS, its call in run_entry, its inputs, output and reference in
op_ref.ENTRIES and its seeds in SEEDS."""

import ctypes
import functools
import re
from pathlib import Path

import torch

import op_ref
from exact_util import MAX_EXCLUDED, bits_of
from gpu_util import DTYPES, assert_op_close, last_kernel, pad16, pad_part, planes_per, q, stream_ptr, to_act, ulp_of
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


def upload(entry, args, dt, inputs):
    """The entry's inputs, logical float CPU tensors by name, as the device tensors of its call: by the roles of tests/op_ref.py."""
    dtype = DTYPES.get(dt, dt)
    op_ref.check_shapes(entry, args, inputs)
    how = {op_ref.ACT: lambda v: to_act(v, dtype), op_ref.IMG: lambda v: v.to("cuda", dtype).contiguous(), op_ref.PAR: dev_w}
    return {name: how[role](inputs[name]) for name, (_, role) in op_ref.inputs(entry, args).items()}


def out_shape(entry, args, dt):
    """Shape of the output's device tensor: plane-major, or the head's dense image."""
    C, logical = op_ref.output(entry, args)
    ppu = planes_per(DTYPES.get(dt, dt))
    return logical if C is None else (logical[0], pad16(C) // ppu, logical[2], logical[3], ppu)


def alloc_out(entry, args, dt, fill=7.0):
    """The output's device tensor, pre-filled with garbage."""
    return torch.full(out_shape(entry, args, dt), fill, dtype=DTYPES.get(dt, dt), device="cuda")


def real(entry, args, out):
    """The real channels of an output, [B, C, Hout, Wout] in its storage type, on the CPU."""
    C = op_ref.output(entry, args)[0]
    if C is None:
        return out.cpu()
    B, P, H, W, ppu = out.shape
    return out.permute(0, 1, 4, 2, 3).reshape(B, P * ppu, H, W)[:, :C].cpu()


def launch(entry, args, dt, inputs, alpha=0.0):
    """The operator on the given data (upload): (output on the GPU, its real channels [B, C, H, W] on the CPU, storage type)."""
    out = alloc_out(entry, args, dt)
    run_entry(entry, args, dt, upload(entry, args, dt, inputs), out, alpha)
    return out, real(entry, args, out)


def check_rounded_once(row, what, ex, out, got):
    """A row of the exact tables (exact_util.Exact) after launch(): equality with the float64 result rounded once (zeros of either sign
    are equal); the elements whose transcendental is not saturated are compared with the one-operator tolerance instead."""
    if row.kernel is not None:
        assert last_kernel() == row.kernel, (last_kernel(), row.kernel)
    want = ex.want
    assert got.shape == want.shape and got.dtype == want.dtype
    assert not bool(torch.isnan(got.float()).any())
    g, w = (got, want) if ex.keep is None else (got[ex.keep], want[ex.keep])
    if not torch.equal(g, w):
        bad = (got != want) if ex.keep is None else (got != want) & ex.keep
        idx = tuple(int(v) for v in bad.nonzero()[0])
        mask = 0xFFFFFFFF if row.dt == "f32" else 0xFFFF
        flushed = int((bad & (got == 0)).sum())
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ from the float64 result rounded once ({flushed} of them are "
                             f"zero); first at {idx}: got {got[idx].item()!r} (bits {bits_of(got[idx].reshape(1)).item() & mask:#x}), want "
                             f"{want[idx].item()!r} (bits {bits_of(want[idx].reshape(1)).item() & mask:#x}), float64 {ex.y64[idx].item()!r}")
    if ex.keep is not None:
        print(f"{what}: excluded share {ex.excluded:.5f} ({int((~ex.keep).sum())} elements)")
        assert ex.excluded <= MAX_EXCLUDED
        assert bool(torch.isfinite(got.float()).all())
        soft = ~ex.keep
        if bool(soft.any()):
            assert_op_close(got.float()[soft], ex.soft64[soft].float(), row.dt, what + " (excluded elements)")
    if ex.C is not None:
        assert bool((pad_part(out, ex.C) == 0).all()), "pad channels must be written as zeros"


# Op's data: seeds in the order of the entry's inputs, the alpha of the mixes, and the parameters that are not q(wrnd(shape, seed))
SEEDS = {"conv": (1, 2), "film": (1, 2, 43, 44), "d2s": (3, 4), "crush": (5, 6), "mix": (7, 8, 9), "conv_mix": (41, 42, 43, 44),
         "stem": (10, 11, 12), "final": (13, 14, 15)}
ALPHA = {"mix": 0.37, "conv_mix": 0.3}


def _parameter(shape, seed, dtype):
    return q(wrnd(shape, seed), dtype)


PARAMETERS = {("film", "gamma"): lambda shape, seed, dtype: 1.0 + 0.5 * rnd(shape, seed),
              ("film", "beta"): lambda shape, seed, dtype: 0.3 * rnd(shape, seed),
              ("stem", "w"): lambda shape, seed, dtype: rnd(shape, seed),
              ("stem", "b"): lambda shape, seed, dtype: rnd(shape, seed, 0.1),
              ("final", "w"): lambda shape, seed, dtype: q(wrnd(shape, seed) * 0.5, dtype)}


class Op:
    """One operator call on seeded O(1) data.  Host side, needs no GPU: `inputs` (float32 CPU tensors by argument name, rounded to the
    storage type where they travel in it), `batched` (the names that hold one entry per image), `C` and `out_shape` of the output,
    `alpha`, the float32 oracle `want` and `tol`.  `t` uploads the inputs when it is first read."""

    def __init__(self, entry, args, dt):
        self.entry, self.args, self.dt = entry, args, dt
        dtype = self.dtype = DTYPES[dt]
        stated = op_ref.inputs(entry, args)
        self.inputs = {}
        for (name, (shape, role)), seed in zip(stated.items(), SEEDS[entry], strict=True):
            if role == op_ref.PAR:
                self.inputs[name] = PARAMETERS.get((entry, name), _parameter)(shape, seed, dtype)
            else:  # an image is not negative
                self.inputs[name] = q(rnd(shape, seed).abs() if role == op_ref.IMG else rnd(shape, seed), dtype)
        self.batched = [name for name, (_, role) in stated.items() if role != op_ref.PAR]
        self.C, self.out_shape = op_ref.output(entry, args)[0], out_shape(entry, args, dt)
        self.alpha = ALPHA.get(entry, 0.0)
        self.tol = None  # element-wise tolerance where it is not gpu_util's one-operator tolerance
        if entry in op_ref.MIXES:
            # the fused kernel rounds z to the storage type before the gate GEMM and the blend, as the unfused path stores it: one
            # rounding of the output plus one rounding step of z where its fp32 sum sits on a boundary (tests/test_conv3r_gpu.py)
            m = op_ref.Mix(entry, self.inputs, lambda z: q(z, dtype))
            self.want = oracle.residual_mix(m.x, m.z, m.w, torch.tensor(self.alpha))
            if entry == "conv_mix":
                self.tol = ulp_of(self.want, dt) + ulp_of(m.z, dt) + 1e-5
        else:
            self.want = op_ref.reference(entry, args, self.inputs)
        assert tuple(self.want.shape) == op_ref.output(entry, args)[1], (entry, args)

    @functools.cached_property
    def t(self):
        """The device tensors by argument name."""
        return upload(self.entry, self.args, self.dt, self.inputs)

    def real(self, out):
        """The output's real channels as float32 [B, C, H, W] on the CPU."""
        return real(self.entry, self.args, out).float()

    def run(self, t, out):
        run_entry(self.entry, self.args, self.dt, t, out, self.alpha)


def select_op(dtype_code, op, cin, cout, B, H, W, cus=256):
    """mz_debug_select: the family the host chooses on `cus` CUs (256: an MI355X), None where it refuses.  Needs no GPU."""
    got = _ffi.lib().mz_debug_select(dtype_code, op, cin, cout, B, H, W, cus)
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
