"""The torch restatement of the dihedral transforms and the self-ensemble arithmetic (include/mewzoom_hip.h, "the dihedral transforms
and the geometric self-ensemble"): the checker of tests/test_dihedral_gpu.py, tests/test_ensemble_gpu.py and
tests/test_poison_ensemble_gpu.py.  Plain torch, wherever the tensors live; nothing of the library is called here."""

import functools

import torch


def T(x, k):
    """Orientation k of x [B, 3, H, W]: bit 1 reverses rows, bit 0 reverses columns, bit 2 exchanges rows and columns, applied last."""
    if k & 2:
        x = x.flip(2)
    if k & 1:
        x = x.flip(3)
    if k & 4:
        x = x.transpose(2, 3)
    return x


def inverse(k):
    return k if k < 4 else 4 | ((k & 1) << 1) | ((k & 2) >> 1)


def bits(t):
    """A tensor as integers of its element width: equality of these is equality of bit patterns (NaN payloads, -0)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def value(y):
    """The `value` of the ensemble: the element as float32; a uint8 sample as the float32 0..255 it is."""
    return y.to(torch.float32)


def accumulate(results, ks):
    """acc_0 = v_0, acc_i = acc_(i-1) + v_i in float32, v_i = value(T(results[i], inverse(ks[i])))."""
    acc = None
    for y, k in zip(results, ks):
        v = value(T(y, inverse(k))).contiguous()
        acc = v if acc is None else acc + v
    return acc


def finish(acc, n, dtype, clamp=True):
    """Float types: acc * (1 / n), the clamp, one rounding to dtype.  uint8: (2 sum + n) / (2 n) in integers."""
    if dtype == torch.uint8:
        s = acc.to(torch.int64)
        assert torch.equal(s.to(torch.float32), acc), "uint8 sums are integers"
        return ((2 * s + n) // (2 * n)).to(torch.uint8)
    v = acc * torch.tensor(1.0 / n, dtype=torch.float32, device=acc.device)
    if clamp:
        v = v.clamp(0.0, 1.0)  # (the tests feed the arithmetic no NaN: fminf / fmaxf and torch.clamp differ on one)
    return v.to(dtype)


def upscale_one(model, x):
    return model.upscale_uint8(x) if x.dtype == torch.uint8 else model.upscale(x)


def ensemble(model, x, n):
    """The composition upscale_ensemble is defined by: model.upscale on contiguous torch-made orientations, each result turned back,
    float32 sums in the order k = 0 .. n - 1, the finish with the clamp."""
    ks = list(range(n))
    results = [upscale_one(model, T(x, k).contiguous()) for k in ks]
    return finish(accumulate(results, ks), n, x.dtype, clamp=True)


# ---- the inputs of tests/test_dihedral_gpu.py, shared with tests/test_poison_ensemble_gpu.py ------------------------------------------------
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.uint8}
INT_OF = {4: torch.int32, 2: torch.int16, 1: torch.uint8}


def shape_id(s):
    return "x".join(str(v) for v in s)


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def random_bits(dt: str, B: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """[B, 3, H, W] of DTYPES[dt] holding random bit patterns; the first elements are NaN, a NaN with a payload, -0, +inf, -inf.
    Shared between the tests and never written to."""
    dtype = DTYPES[dt]
    size = torch.empty((), dtype=dtype).element_size()
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + 31 * H + W)
    raw = torch.randint(0, 256, (B * 3 * H * W * size,), dtype=torch.uint8, device="cuda", generator=g)
    x = raw.view(dtype).view(B, 3, H, W)
    if dt != "u8":
        special = torch.tensor([float("nan"), float("nan"), -0.0, float("inf"), float("-inf")], dtype=dtype, device="cuda")
        n = min(5, W)
        x[0, 0, 0, :n] = special[:n]
        if W > 1:
            x.view(INT_OF[size])[0, 0, 0, 1] |= 0x15  # a payload in the second NaN
    else:
        x.view(-1)[: min(2, x.numel())] = torch.tensor([0, 255], dtype=torch.uint8, device="cuda")[: min(2, x.numel())]
    return x


@functools.lru_cache(maxsize=None)
def pass_results(dt: str, B: int, H: int, W: int):
    """Eight pass results of a [B, 3, H, W] ensemble, result k in orientation k's shape.  Float data: normal(0.5, 1), so a good part lies
    outside [0, 1]; uint8: every sample value, 0 and 255 planted."""
    g = torch.Generator(device="cuda").manual_seed(7 * H + W)
    out = []
    for k in range(8):
        h, w = (W, H) if k & 4 else (H, W)
        if dt == "u8":
            y = torch.randint(0, 256, (B, 3, h, w), dtype=torch.uint8, device="cuda", generator=g)
            y.view(-1)[0] = 255 if k & 1 else 0
        else:
            y = (torch.randn((B, 3, h, w), device="cuda", generator=g) + 0.5).to(DTYPES[dt])
        out.append(y)
    return out
