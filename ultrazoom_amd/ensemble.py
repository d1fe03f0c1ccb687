"""The eight orientations of an image and the geometric self-ensemble on the MI355X: `mz_dihedral`, `mz_ensemble_add` and
`mz_ensemble_finish` (include/mewzoom_hip.h) behind a tensor interface.

The self-ensemble is the "+" variant of the super-resolution papers: the model upscales the 8 orientations of the input (4 flips, each
with and without transposition), every result is turned back, the results are averaged.  The reference trains with a horizontal flip only
(pretrain.py:148), so the network is close to equivariant but not exactly and the passes do differ.  No reference counterpart in model.py.

Orientation k = 0..7: bit 0 reverses columns, bit 1 reverses rows, bit 2 exchanges rows and columns and is applied last --
`x.flip(2) if k & 2`, `.flip(3) if k & 1`, `.transpose(2, 3) if k & 4`.  The transform moves elements and never changes them.  Turning a
result back and accumulating it is ONE pass over memory in HIP (a tile transposition through LDS, coalesced on both sides); nothing here
synchronises with the host."""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _ffi

ORIENTATIONS = (1, 2, 4, 8)  # the ensembles there are: the identity; + the mirror; the four flips; the whole group
DEFAULT_WORKSPACE_BYTES = 4 << 30


def dihedral_inverse(k: int) -> int:
    """The orientation that undoes orientation k: k itself for the flips (k < 4) and the two diagonal mirrors (4, 7); the quarter
    turns 5 and 6 undo each other."""
    inv = _ffi.dihedral_inverse(k)
    if inv < 0:
        raise ValueError(f"an orientation is 0..7, got {k}")
    return inv


def dihedral(x: Tensor, k: int, out: Optional[Tensor] = None) -> Tensor:
    """Orientation k of a logical [B, 3, H, W] CUDA tensor (any strides; float32 / bfloat16 / float16 / uint8): a new dense NCHW tensor,
    or `out` ([B, 3, W, H] when k & 4, else [B, 3, H, W]; any strides, x's dtype), bit pattern for bit pattern.  x and out must not
    overlap."""
    elem, B, H, W = _ffi.check_image_batch(x, "dihedral")
    k = int(k)
    if not 0 <= k <= 7:
        raise ValueError(f"an orientation is 0..7, got {k}")
    with _ffi.image_frame(x, out, (B, 3, W, H) if k & 4 else (B, 3, H, W)) as (out, _, stream):
        _ffi.dihedral(*_ffi.pair(x), *_ffi.pair(out), elem, B, H, W, k, stream)
    return out


def plan_chunks(B: int, H: int, W: int, elem_bytes: int, workspace_bytes: int) -> List[Tuple[int, int]]:
    """How `upscale_ensemble` walks a batch of B results of H x W pixels (the sizes of the RESULT) whose elements take `elem_bytes`:
    [(first image, images), ...], as few chunks as `workspace_bytes` allows, no chunk larger than the first.  An image of a chunk costs its
    float32 accumulator plus its place in the pass scratch: 3 H W (4 + elem_bytes) bytes.  A pure function; a budget below one image is
    refused."""
    B, H, W, elem_bytes, workspace_bytes = int(B), int(H), int(W), int(elem_bytes), int(workspace_bytes)
    if B < 1 or H < 1 or W < 1 or elem_bytes not in (1, 2, 4):
        raise ValueError(f"need B, H, W >= 1 and elements of 1, 2 or 4 bytes, got {(B, H, W, elem_bytes)}")
    per_image = 3 * H * W * (4 + elem_bytes)
    if workspace_bytes < per_image:
        raise ValueError(f"workspace_bytes = {workspace_bytes} is below the {per_image} bytes one {H} x {W} result takes "
                         "(float32 accumulator + pass scratch)")
    per_chunk = min(B, workspace_bytes // per_image)
    return [(b0, min(per_chunk, B - b0)) for b0 in range(0, B, per_chunk)]


@torch.inference_mode()
def upscale_ensemble(model, x: Tensor, n: int = 8, out: Optional[Tensor] = None, tile: Optional[Tuple[int, int]] = None,
                     workspace_bytes: int = DEFAULT_WORKSPACE_BYTES) -> Tensor:
    """The self-ensemble of `model.upscale` (`model.upscale_uint8` for uint8 tensors) over the orientations k = 0 .. n - 1:

        mean over k of T(U(T(x, k)), inverse(k)),   clamped to [0, 1]

    n = 1 is `upscale` itself (the same bits), 2 is {identity, mirror}, 4 the four flips (no shape changes), 8 the whole group.  Each
    pass is `model.upscale` of that orientation of x, bit for bit; its result lies in one scratch tensor that every pass reuses, and is
    turned back and added to a float32 accumulator in one HIP pass over memory.  Float types: float32 sums in the order of k, times 1 / n
    (exact), the clamp, one rounding to x's dtype.  uint8: integer sums of the samples, (2 sum + n) / (2 n): round half up.

    x: a logical [B, 3, H, W] CUDA tensor of the model's dtype or uint8, any strides.  `out` ([B, 3, rH, rW], any strides, x's dtype)
    receives the result in place.  `tile` = (th, tw) sends every pass through `tiling.upscale_tiled` with that core size.  The batch is
    walked in chunks of images so that accumulator plus pass scratch stay within `workspace_bytes` (default 4 GiB: seven 8K results in
    bfloat16; `plan_chunks`); the result does not depend on the chunking."""
    elem, B, H, W = _ffi.check_image_batch(x, "upscale_ensemble")
    n = int(n)
    if n not in ORIENTATIONS:
        raise ValueError(f"n is 1, 2, 4 or 8 orientations, got {n}")
    r = model.upscale_ratio
    Ho, Wo = r * H, r * W

    def run(xk: Tensor, dst: Tensor) -> None:  # one pass: dst = U(xk)
        if tile is None:
            model.upscale_into(xk, dst)
        else:
            from .tiling import upscale_tiled

            upscale_tiled(model, xk, tile, out=dst)

    with _ffi.image_frame(x, out, (B, 3, Ho, Wo)) as (out, _, stream):
        if n == 1:
            run(x, out)
            return out
        chunks = plan_chunks(B, Ho, Wo, x.element_size(), workspace_bytes)
        b_max = chunks[0][1]
        acc = torch.empty(b_max * 3 * Ho * Wo, dtype=torch.float32, device=x.device)
        scratch = torch.empty(b_max * 3 * Ho * Wo, dtype=x.dtype, device=x.device)   # the one pass result there ever is
        turned = torch.empty(b_max * 3 * H * W, dtype=x.dtype, device=x.device)      # the orientation of the (small) input
        for b0, nb in chunks:
            xc, oc = x[b0:b0 + nb], out[b0:b0 + nb]
            acc_bytes = _ffi.ensemble_workspace_bytes(nb, Ho, Wo)
            for k in range(n):
                hk, wk = (W, H) if k & 4 else (H, W)
                xk = xc if k == 0 else dihedral(xc, k, out=turned[: nb * 3 * hk * wk].view(nb, 3, hk, wk))
                yk = scratch[: nb * 3 * Ho * Wo].view(nb, 3, r * hk, r * wk)
                run(xk, yk)
                _ffi.ensemble_add(*_ffi.pair(yk), elem, nb, Ho, Wo, k, k == 0, acc.data_ptr(), acc_bytes, stream)
            _ffi.ensemble_finish(*_ffi.pair(oc), elem, nb, Ho, Wo, n, True, None, acc.data_ptr(), acc_bytes, stream)
    return out
