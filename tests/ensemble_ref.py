"""The torch restatement of the dihedral transforms and the self-ensemble arithmetic (include/mewzoom_hip.h, "the dihedral transforms
and the geometric self-ensemble"): the checker of tests/test_dihedral_gpu.py, tests/test_ensemble_gpu.py and
tests/test_poison_ensemble_gpu.py.  Plain torch, wherever the tensors live; nothing of the library is called here."""

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
