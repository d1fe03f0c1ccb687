"""upscale_ensemble / MewZoom.upscale_ensemble on the GPU against the composition of tests/ensemble_ref.py: `model.upscale` on contiguous
torch-made orientations, every result turned back by torch, float32 sums in the order k = 0 .. n - 1, the finish as the header states
it.  Every comparison with that composition is `torch.equal`; the equivariance bounds are derived where they are used.

Models are the tiny fixtures of tests/golden: g1_2x_c16 at LR 13 x 22 with three images, g3_4x_c16 at 8 x 9 with two; "u8" runs uint8
images through the bf16 model."""

import functools

import pytest
import torch

import ensemble_ref as ref
from golden_util import GoldenCase
from ultrazoom_amd import MewZoom, upscale_ensemble
from ultrazoom_amd.ensemble import plan_chunks
from ultrazoom_amd.synth import synth_image

pytestmark = pytest.mark.gpu

MODEL_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "u8": torch.bfloat16}
KINDS = sorted(MODEL_DTYPE)
CASES = [("g1_2x_c16", 3, 13, 22), ("g3_4x_c16", 2, 8, 9)]
INT_OF = {4: torch.int32, 2: torch.int16}


def case_id(c):
    return f"{c[0]}_{c[1]}x{c[2]}x{c[3]}"


@functools.lru_cache(maxsize=None)
def model(name: str, kind: str) -> MewZoom:
    case = GoldenCase(name)
    m = MewZoom(**case.config)
    m.load_state_dict(case.weights())
    return m.to("cuda", MODEL_DTYPE[kind]).eval()


@functools.lru_cache(maxsize=None)
def image(kind: str, B: int, H: int, W: int, seed: int = 11) -> torch.Tensor:
    """Shared and never written to."""
    x = synth_image(B, H, W, seed=seed)
    if kind == "u8":
        return (x * 255.0).round().to(torch.uint8).cuda()
    return x.to("cuda", MODEL_DTYPE[kind])


@functools.lru_cache(maxsize=None)
def composed(name: str, kind: str, B: int, H: int, W: int, n: int) -> torch.Tensor:
    """The torch composition, computed once per case."""
    return ref.ensemble(model(name, kind), image(kind, B, H, W), n)


@functools.lru_cache(maxsize=None)
def ensembled(name: str, kind: str, B: int, H: int, W: int, n: int) -> torch.Tensor:
    """upscale_ensemble with its defaults, computed once per case."""
    return model(name, kind).upscale_ensemble(image(kind, B, H, W), n=n)


@pytest.mark.parametrize("n", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ensemble_is_the_torch_composition(case, kind, n):
    name, B, H, W = case
    m, x = model(name, kind), image(kind, B, H, W)
    got = ensembled(name, kind, B, H, W, n)
    r = m.upscale_ratio
    assert got.shape == (B, 3, r * H, r * W) and got.dtype == x.dtype and got.is_contiguous()
    assert torch.equal(got, composed(name, kind, B, H, W, n))
    if n == 1:
        assert torch.equal(got, ref.upscale_one(m, x))
    else:
        assert not torch.equal(got, ref.upscale_one(m, x)), "the passes of the other orientations changed nothing"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_pass_is_upscale_of_that_orientation(case, kind):
    """What upscale_ensemble feeds the model -- mz_dihedral's copy of the orientation, through upscale_into -- gives the bits of
    `model.upscale` on torch's contiguous orientation."""
    from ultrazoom_amd import dihedral

    name, B, H, W = case
    m, x = model(name, kind), image(kind, B, H, W)
    r = m.upscale_ratio
    for k in range(8):
        xk = dihedral(x, k)
        out = torch.empty((B, 3, r * xk.shape[2], r * xk.shape[3]), dtype=x.dtype, device="cuda")
        assert torch.equal(m.upscale_into(xk, out), ref.upscale_one(m, ref.T(x, k).contiguous())), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_chunking_tiling_and_layouts_do_not_change_the_bits(case, kind):
    name, B, H, W = case
    m, x = model(name, kind), image(kind, B, H, W)
    r = m.upscale_ratio
    for n in (2, 8):
        want = ensembled(name, kind, B, H, W, n)
        # one image per chunk
        one = 3 * r * H * r * W * (4 + x.element_size())
        assert plan_chunks(B, r * H, r * W, x.element_size(), one) == [(b, 1) for b in range(B)]
        assert torch.equal(upscale_ensemble(m, x, n=n, workspace_bytes=one), want)
        with pytest.raises(ValueError, match="below"):
            upscale_ensemble(m, x, n=n, workspace_bytes=one - 1)
        # every pass through upscale_tiled
        assert torch.equal(m.upscale_ensemble(x, n=n, tile=(16, 16)), want)
        # a channels-last input and a strided out: a crop of a larger channels-last frame
        frame = torch.full((B, 3, r * H + 5, r * W + 7), 77, dtype=x.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
        out = frame[:, :, 2 : 2 + r * H, 3 : 3 + r * W]
        assert m.upscale_ensemble(x.contiguous(memory_format=torch.channels_last), n=n, out=out) is out
        assert torch.equal(out, want)
        out.fill_(77)
        assert bool((frame == 77).all()), "stores outside out"
    out = torch.empty_like(want)
    assert m.upscale_ensemble(x, n=1, out=out) is out and torch.equal(out, ref.upscale_one(m, x))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_uint8_ensemble_of_the_whole_group_is_exactly_equivariant(case):
    """upscale_ensemble(T(x, j)) == T(upscale_ensemble(x), j): the 8 passes are the same set, integer sums do not depend on their order,
    the finish is element-wise."""
    name, B, H, W = case
    m, x = model(name, "u8"), image("u8", B, H, W)
    base = ensembled(name, "u8", B, H, W, 8)
    for j in range(8):
        assert torch.equal(m.upscale_ensemble(ref.T(x, j).contiguous(), n=8), ref.T(base, j)), j


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_float_ensemble_of_the_whole_group_is_equivariant_up_to_the_order_of_the_sums(case, kind):
    """The two sides add the same eight float32 values of [0, 1] in two orders.  A sum of eight such values makes 7 roundings of at most
    8 * 2^-24 each; after the 1 / 8 that is 7 * 2^-24 = 4.2e-7 an order, below 1e-6 for the two -- the f32 bound.  That error is also
    relative (the summands are not negative, so every partial sum is at most the total): 7 * 2^-23 of the mean, far inside the 2^-8 /
    2^-11 spacing of bf16 / f16, so the two roundings to the stored type land on the same value or on neighbours: at most one unit in
    the last place, measured on the bit patterns (the values are not negative: their order is the order of their patterns)."""
    name, B, H, W = case
    m, x = model(name, kind), image(kind, B, H, W)
    base = ensembled(name, kind, B, H, W, 8)
    worst = 0
    for j in range(8):
        got, want = m.upscale_ensemble(ref.T(x, j).contiguous(), n=8), ref.T(base, j).contiguous()
        assert got.shape == want.shape
        if kind == "f32":
            diff = float((got - want).abs().max())
            worst = max(worst, diff)
            assert diff < 1e-6, (j, diff)
        else:
            steps = (got.abs().view(INT_OF[2]).to(torch.int32) - want.abs().view(INT_OF[2]).to(torch.int32)).abs().max()
            worst = max(worst, int(steps))
            assert int(steps) <= 1, (j, int(steps))
    print(f"{name} {kind}: worst difference between the two orders: {worst}" + ("" if kind == "f32" else " unit(s) in the last place"))


def test_evaluate_with_an_ensemble_measures_the_ensemble_outputs():
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr
    from ultrazoom_amd.metrics import MetricsAccumulator

    name, B, H, W = CASES[0]
    m = model(name, "bf16")
    batches = [(image("bf16", B, H, W), synth_image(B, 2 * H, 2 * W, seed=5).to("cuda", torch.bfloat16)),
               (image("bf16", 1, H, W, seed=12), synth_image(1, 2 * H, 2 * W, seed=6).to("cuda", torch.bfloat16))]
    for n in (8, 2):
        acc = MetricsAccumulator(1.0)
        for x, y in batches:
            acc.update(upscale_ensemble(m, x, n=n), y)
        want = acc.compute()
        got = evaluate(m, batches, backend="hip", ensemble=n)
        assert got == {**want, "images": B + 1}, (n, got, want)
        plain = evaluate(m, batches, backend="hip")
        assert plain == evaluate(m, batches, backend="hip", ensemble=1) and plain["psnr"] != got["psnr"]
    # evaluate_hr hands the keyword on
    hr = [synth_image(2, 48, 64, seed=9).to("cuda", torch.bfloat16)]
    from ultrazoom_amd.evaluate import lr_from_hr

    pairs = [lr_from_hr(h, 2, "bicubic", "hip") for h in hr]
    assert evaluate_hr(m, hr, backend="hip", ensemble=4) == evaluate(m, pairs, backend="hip", ensemble=4)


def test_evaluate_hr_with_a_degradation_and_an_ensemble():
    """The blind-degradation recipe with ensemble > 1: the image metrics are those of the ensemble on the degraded pairs, the quality
    head's error is that of one plain pass."""
    from ultrazoom_amd import Degradation
    from ultrazoom_amd.evaluate import evaluate, evaluate_hr

    m = model(CASES[0][0], "bf16")
    deg = Degradation(seed=0)
    batches = [synth_image(2, 96, 112, seed=9).to("cuda", torch.bfloat16), synth_image(1, 96, 112, seed=10).to("cuda", torch.bfloat16)]
    got = evaluate_hr(m, batches, backend="hip", degrade=deg, ensemble=4)
    pairs, sq, count, n = [], 0.0, 0, 0
    for hr in batches:
        lr, target, want_qa = deg.apply(hr, m.upscale_ratio, index=n)
        pairs.append((lr, target))
        qa = m.forward(lr)[1]
        sq += float(((qa.double().cpu() - want_qa.double().cpu()) ** 2).sum())
        count += qa.numel()
        n += hr.shape[0]
    want = evaluate(m, pairs, backend="hip", ensemble=4)
    assert got["images"] == 3 and {k: got[k] for k in want} == want
    assert abs(got["deg_l2"] - sq / count) <= 1e-12 * max(1.0, sq / count)
    assert got["psnr"] != evaluate_hr(m, batches, backend="hip", degrade=deg)["psnr"]
    with pytest.raises(ValueError, match="ensemble"):
        evaluate_hr(m, batches, backend="hip", degrade=deg, ensemble=3)
