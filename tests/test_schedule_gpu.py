"""What mz_debug_schedule() says is what mz_forward launches: the handle's profiler records every 3x3, mix and PixelCrush launch, and its
dump must be the schedule's steps of those kinds, micro-batch after micro-batch.  37 x 45 floors to 18 x 22, 9 x 11 and 4 x 5 (every zero
border and crop is live), C = 16 fuses the blocks of levels 0 to 2 and not those of level 3, 8X has all three head buffers."""

import csv

import pytest
import torch

from golden_util import GoldenCase
from model_util import build
from ultrazoom_amd.synth import synth_image

pytestmark = pytest.mark.gpu

KINDS = {1: "conv3", 2: "mix", 3: "crush"}  # mz_debug_step.kind -> the dump's name


@pytest.mark.parametrize("want_qa", [True, False], ids=["forward", "upscale"])
@pytest.mark.parametrize("name", ["g1_2x_c16", "g3_4x_c16", "g4_8x_c16"])
def test_profiled_launches_are_the_schedule(name, want_qa, tmp_path):
    case = GoldenCase(name)
    m = build(case, case.weights(), torch.bfloat16)
    m.max_images_in_flight = 1
    B, H, W = 2, 37, 45
    x = synth_image(B, H, W, 5).to("cuda", torch.bfloat16)
    run = m.forward if want_qa else m.upscale
    run(x)  # makes the handle
    handle = m._engine.handle
    handle.profile_enable(True)
    run(x)
    torch.cuda.synchronize()
    handle.profile_dump(tmp_path / "launches.csv")
    handle.profile_enable(False)
    with open(tmp_path / "launches.csv") as f:
        got = [(r["kind"],) + tuple(int(r[k]) for k in ("B", "H", "W", "cin", "cout")) for r in csv.DictReader(f)]
    steps = handle.schedule(1, H, W, want_qa)
    one = [(KINDS[s["kind"]], s["B"], s["H"], s["W"], s["cin"], s["cout"]) for s in steps if s["kind"] in KINDS]
    assert {k for k, *_ in one} == set(KINDS.values()) and len(one) >= 25
    assert any(s["fused"] for s in steps) and any(s["kind"] == 2 and s["H"] == 4 for s in steps)  # fused blocks, and level 3's unfused ones
    assert got == one * B
