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

import pytest
import torch

from gpu_util import DTYPES, assert_op_close, last_kernel, pad16
from op_cases import CASES, FAMILY_OF_UNREPORTED, case_id, select_args
from op_util import Op, kernel_names, selected, set_knobs
from poison_util import Arena


def test_the_case_table_names_every_kernel_family():
    """Needs no GPU: every literal kernel_name() (mz_select.h) can return is the expected kernel of some row, so that a family added
    later cannot be forgotten here."""
    names = kernel_names()
    covered = {c[4] for c in CASES if c[4]} | {FAMILY_OF_UNREPORTED[c[0]] for c in CASES if c[0] in FAMILY_OF_UNREPORTED}
    assert names <= covered, f"no row of CASES runs {sorted(names - covered)}"
    assert all(c[3] in DTYPES for c in CASES)
    assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", [c for c in CASES if select_args(c[0], c[1]) is not None], ids=case_id)
def test_the_expected_kernels_are_the_host_s_choice(case, monkeypatch):
    """Needs no GPU: the expected name of every row is what choose_conv3 / choose_mix choose on an MI355X (256 CUs)."""
    entry, args, env, dt, kernel = case
    set_knobs(monkeypatch, env)
    got = selected(entry, args, dt)
    assert got is not None and got == kernel, (got, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_poisoned_surroundings(case, monkeypatch):
    entry, args, env, dt, kernel = case
    set_knobs(monkeypatch, env)
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
