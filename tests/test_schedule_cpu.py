"""The forward pass as the library states it (mz_schedule.h: make_schedule), read without a GPU through mz_debug_schedule(): the steps of
one micro-batch in launch order, each with its shapes and its operands as workspace offsets.  mz_forward runs exactly these steps, so
what is checked here -- no step reads a buffer that another has overwritten, every operand fits its slot of the workspace, the table of
tests/test_select_cpu.py lists the layers that are launched, the flops -- is checked of the code the model runs."""

import re
from pathlib import Path

import pytest

import bench
from golden_util import GoldenCase
from op_util import set_knobs
from ultrazoom_amd import _ffi

F32, BF16, F16 = _ffi.MZ_F32, _ffi.MZ_BF16, _ffi.MZ_F16
STEM, CONV3, MIX, CRUSH, ZERO_BORDER, QA_REDUCE = range(6)  # mz_debug_step.kind
CONV1, CONV, UP, HEAD, QA, FILM, CONV2, MIXOP = range(8)    # mz_debug_step.op: mz_debug_select's
NONE, IMAGE_IN, IMAGE_OUT, QA_OUT = -1, -2, -3, -4          # mz_debug_step.off of an operand outside the workspace
CUS = 256  # MI355X

# 2X, 4X, 8X (one, two, three head levels); C = 16, 24, 32; hidden ratio 1, 2, 4
FIXTURES = ["g1_2x_c16", "g3_4x_c16", "g4_8x_c16", "g8_c24_f5", "g9_4x_c32", "g5_hr1", "g5_hr4"]
SIZES = [(8, 8), (37, 45), (64, 120)]


def pad16(c):
    return (c + 15) // 16 * 16


def micro_batch(h, B, H, W):
    """The default micro-batch of B images: the one whose workspace mz_workspace_bytes reports."""
    return next(n for n in range(1, B + 1) if h.workspace_bytes(n, H, W, n) == h.workspace_bytes(B, H, W, 0))


def plan_slots(cfg, sz, nb, H, W):
    """{offset: bytes} of the workspace's buffers and their total, bump-allocated in 256-byte steps as make_plan (mz_plan.h) does:
    per level three feature buffers, the hidden tensor, z and (levels 0..2) the up-sampled tensor; per further head level two feature
    buffers, hidden, z; the quality head's features."""
    ch = [cfg[f"{n}_channels"] for n in ("primary", "secondary", "tertiary", "quaternary")]
    hr, nhead = cfg["hidden_ratio"], {2: 1, 4: 2, 8: 3}[cfg["upscale_ratio"]]
    slots, off = {}, 0

    def take(nbytes):
        nonlocal off
        slots[off] = nbytes
        off += (nbytes + 255) // 256 * 256

    h, w = H, W
    for l in range(4):
        c = nb * h * w * pad16(ch[l]) * sz
        for nbytes in (c, c, c, nb * h * w * pad16(hr * ch[l]) * sz, c) + ((c,) if l < 3 else ()):
            take(nbytes)
        last = (h, w)
        h, w = h // 2, w // 2
    for j in range(1, nhead):
        px = nb * (H << j) * (W << j)
        for nbytes in (px * pad16(ch[0]) * sz,) * 2 + (px * pad16(hr * ch[0]) * sz, px * pad16(ch[0]) * sz):
            take(nbytes)
    take(nb * last[0] * last[1] * pad16(cfg["num_deg_features"]) * sz)
    return slots, off


def check_schedule(h, cfg, dtype, nb, H, W, want_qa):
    sz = 4 if dtype == F32 else 2
    steps = h.schedule(nb, H, W, want_qa, CUS)
    slots, total = plan_slots(cfg, sz, nb, H, W)
    assert total == h.workspace_bytes(nb, H, W, nb)  # the slots are the library's
    r, F = cfg["upscale_ratio"], cfg["num_deg_features"]
    image = nb * 3 * H * W * sz

    def act(hh, ww, c):
        return nb * hh * ww * pad16(c) * sz

    live = set()  # (begin, end) of the tensors in the workspace
    for i, s in enumerate(steps):
        what = (i, s)
        kind, op, cin, cout, hh, ww = s["kind"], s["op"], s["cin"], s["cout"], s["H"], s["W"]
        (in0, in1, out), (n0, n1, nout) = s["off"], s["bytes"]
        assert s["B"] == nb
        # ---- extents: what the shapes say
        if kind == STEM:
            want = ((IMAGE_IN, image), (NONE, 0), act(hh, ww, cout))
        elif kind == CONV3 and op == HEAD:
            assert (s["Hout"], s["Wout"]) == (2 * hh, 2 * ww) == (r * H, r * W), what
            want = (act(hh, ww, cin), (IMAGE_IN, image), (IMAGE_OUT, nb * 3 * s["Hout"] * s["Wout"] * sz))
        elif kind == CONV3 and op == UP:
            assert s["Hout"] // 2 == hh and s["Wout"] // 2 == ww and cout % 4 == 0, what
            want = (act(hh, ww, cin), (NONE, 0), act(s["Hout"], s["Wout"], cout // 4))
        elif kind == CONV3:
            assert op in (CONV1, CONV2, QA) and (s["fused"] == 0 or op == CONV2), what
            want = (act(hh, ww, cin), act(hh, ww, cout) if s["fused"] else (NONE, 0), act(hh, ww, cout))
        elif kind == MIX:
            assert op == MIXOP and cin == 2 * cout, what
            want = (act(hh, ww, cout),) * 3
        elif kind == CRUSH:
            assert (s["Hout"], s["Wout"]) == (hh // 2, ww // 2), what
            want = (act(hh, ww, cin), (NONE, 0), act(s["Hout"], s["Wout"], cout))
        elif kind == ZERO_BORDER:
            assert in0 == out, what  # in place
            want = (act(s["Hout"], s["Wout"], cout // 4), (NONE, 0), act(s["Hout"], s["Wout"], cout // 4))
        else:
            assert kind == QA_REDUCE and cout == F, what
            want = (act(hh, ww, F), (NONE, 0), (QA_OUT, nb * F * 4))
        assert (op >= 0) == (kind in (CONV3, MIX)) == (s["kernel"] is not None), what
        for (off, nbytes), w in zip(((in0, n0), (in1, n1), (out, nout)), want):
            if isinstance(w, tuple):  # outside the workspace
                assert (off, nbytes) == w, what
            else:  # inside: in one slot of the plan, which holds it
                assert nbytes == w and off in slots and nbytes <= slots[off] and 0 <= off and off + nbytes <= total, what
        # ---- liveness
        reads = [(o, o + n) for o, n in ((in0, n0), (in1, n1)) if o >= 0]
        for rd in reads:
            assert rd in live, ("reads what no earlier step left there", what)
        if out >= 0:
            wr = (out, out + nout)
            if kind != ZERO_BORDER:
                assert all(wr[1] <= a or b <= wr[0] for a, b in reads), ("writes over its own input", what)
            live = {t for t in live if wr[1] <= t[0] or t[1] <= wr[0]} | {wr}
    assert steps[0]["kind"] == STEM and steps[0]["off"][0] == IMAGE_IN
    assert steps[-1]["op"] == HEAD and steps[-1]["off"][1:] == (IMAGE_IN, IMAGE_OUT)
    assert [s["kind"] for s in steps].count(QA_REDUCE) == (1 if want_qa else 0) == sum(s["op"] == QA for s in steps)
    return steps


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_schedules_are_live_and_fit(name, size, monkeypatch):
    set_knobs(monkeypatch)
    cfg = GoldenCase(name).config
    for dtype in (BF16, F32):
        h = _ffi.Handle(cfg, dtype)
        for want_qa in (True, False):
            for nb in (1, 2):
                check_schedule(h, cfg, dtype, nb, *size, want_qa)
        h.close()


@pytest.mark.parametrize("workload", list(bench.WORKLOADS))
def test_bench_schedules_are_live_and_fit(workload, monkeypatch):
    set_knobs(monkeypatch)
    model, B, H, W, _ = bench.WORKLOADS[workload]
    cfg = bench.MODELS[model]
    for dtype in (BF16, F32):
        h = _ffi.Handle(cfg, dtype)
        for want_qa in (True, False):
            check_schedule(h, cfg, dtype, micro_batch(h, B, H, W), H, W, want_qa)
        h.close()


def test_an_overwritten_input_is_noticed(monkeypatch):
    """check_schedule's own liveness rule on a schedule with two steps swapped: the later step's input is not there yet."""
    set_knobs(monkeypatch)
    cfg = GoldenCase("g3_4x_c16").config
    h = _ffi.Handle(cfg, BF16)
    steps = h.schedule(1, 37, 45, True, CUS)
    real = h.schedule
    # a step whose output the next one is the first to read in a buffer nobody wrote before: the first conv1, each sub-pixel conv
    first_writes = [1] + [i for i in range(len(steps) - 1) if steps[i + 1]["kind"] == ZERO_BORDER]
    assert len(first_writes) == 4 and steps[1]["op"] == CONV1 and steps[2]["off"][0] == steps[1]["off"][2]
    for i in first_writes:
        swapped = steps[:i] + [steps[i + 1], steps[i]] + steps[i + 2:]
        h.schedule = lambda *a: swapped
        with pytest.raises(AssertionError):
            check_schedule(h, cfg, BF16, 1, 37, 45, True)
    h.schedule = real
    h.close()


# ---- the hand table of tests/test_select_cpu.py ---------------------------------------------------
def _c(ratio, ch, layers=(2, 2, 2, 2)):
    cfg = {"upscale_ratio": ratio, "hidden_ratio": 2, "num_deg_features": 3}
    for n, c, l in zip(("primary", "secondary", "tertiary", "quaternary"), ch, layers):
        cfg[f"{n}_channels"], cfg[f"{n}_layers"] = c, l
    return cfg


C16, C24, C32 = (16, 32, 64, 128), (24, 40, 72, 136), (32, 64, 128, 256)
# heading of TABLE -> (model, dtype, images, H, W[, micro-batch where the rows are not at the default one]).  "cfg3_1080p, f32" has its rows
# at the three images of the 16-bit headings; f32 tensors are twice the size and the default micro-batch is ONE image, which the test
# below holds to the same kernels.  The fixture headings: the fixtures' channel widths (g1 / g3, g8, g9) with three quality
# features, as a 4X model on the odd 37 x 45 image and as a 2X model on two 64 x 120 images
HEADINGS = {
    "cfg3_1080p, bf16, the default micro-batch of 3 images": (bench.MODELS["4x96"], BF16, 16, 1080, 1920),
    "cfg3_540p, bf16, the default micro-batch of 15 images": (bench.MODELS["4x96"], BF16, 16, 540, 960),
    "cfg2, bf16, 32 images": (bench.MODELS["2x48"], BF16, 32, 540, 960),
    "cfg3_1080p, f16": (bench.MODELS["4x96"], F16, 16, 1080, 1920),
    "cfg3_1080p, f32": (bench.MODELS["4x96"], F32, 16, 1080, 1920, 3),
    "cfg2, f32": (bench.MODELS["2x48"], F32, 32, 540, 960),
    "fixture models, C = 16, 37 x 45 (bf16)": (_c(4, C16), BF16, 1, 37, 45),
    "fixture models, C = 16, 64 x 120 (f16)": (_c(2, C16), F16, 2, 64, 120),
    "fixture models, C = 24, 37 x 45 (bf16)": (_c(4, C24), BF16, 1, 37, 45),
    "fixture models, C = 24, 64 x 120 (f16)": (_c(2, C24), F16, 2, 64, 120),
    "fixture models, C = 32, 37 x 45 (bf16)": (_c(4, C32, (2, 2, 2, 4)), BF16, 1, 37, 45),
    "fixture models, C = 32, 64 x 120 (f16)": (_c(2, C32, (2, 2, 2, 4)), F16, 2, 64, 120),
}


def table_by_heading():
    """The rows of TABLE (tests/test_select_cpu.py) under each of its comment headings, read from the source: {heading: [row, ..]}."""
    src = (Path(__file__).resolve().parent / "test_select_cpu.py").read_text()
    body = src[src.index("\nTABLE = [\n") + len("\nTABLE = [\n"):src.index("\n]\n", src.index("\nTABLE = [\n"))]
    names = dict(F32=F32, BF16=BF16, F16=F16, CONV1=CONV1, CONV=CONV, UP=UP, HEAD=HEAD, QA=QA, FILM=FILM, CONV2=CONV2, MIX=MIXOP)
    out, heading = {}, None
    for line in body.splitlines():
        line = line.strip()
        if line.startswith("#"):
            heading = line[1:].strip()
            out[heading] = []
        elif line:
            assert re.fullmatch(r"\([A-Z0-9]+, [A-Z0-9]+, [\w ,'=]+\),", line), line
            out[heading].append(eval(line.rstrip(","), {"__builtins__": {}}, names))
    return out


def test_every_model_heading_of_the_table_is_checked():
    headings = table_by_heading()
    assert sum(len(rows) for rows in headings.values()) >= 250
    assert {t for t in headings if t.startswith(("cfg", "fixture models"))} == set(HEADINGS)


@pytest.mark.parametrize("heading", list(HEADINGS))
def test_table_lists_the_layers_the_schedule_launches(heading, monkeypatch):
    """Under a model's heading: one row for every distinct (dtype, op, cin, cout, B, H, W) among the 3x3 / mix steps of that model's
    forward pass, none else, and the kernel the row names is the one the schedule names."""
    set_knobs(monkeypatch)
    cfg, dtype, B, H, W, *nb = HEADINGS[heading]
    rows = table_by_heading()[heading]
    assert all(r[7] == "" for r in rows)
    h = _ffi.Handle(cfg, dtype)

    def launched(nb):
        return {(dtype, s["op"], s["cin"], s["cout"], s["B"], s["H"], s["W"]): s["kernel"] for s in h.schedule(nb, H, W, True, CUS) if s["op"] >= 0}

    default = launched(micro_batch(h, B, H, W))
    got = launched(nb[0]) if nb else default
    h.close()
    want = {r[:7]: r[8] for r in rows}
    assert len(want) == len(rows), "a row twice"
    assert sorted(got) == sorted(want)
    assert got == want
    assert {k[:4] + k[5:]: v for k, v in default.items()} == {k[:4] + k[5:]: v for k, v in want.items()}  # whatever the micro-batch


# ---- flops ----------------------------------------------------------------------------------------
# mz_flops_per_image of the commit before the schedule existed (a closed formula over the configuration), bf16
PARENT_FLOPS = {
    ("4x96", 1080, 1920): 69430249267200,  # cfg3_1080p
    ("4x96", 540, 960): 17313110691840,    # cfg3_540p
    ("2x48", 540, 960): 2063869839360,     # cfg2
    ("g7_cfg1_2x_c48", 256, 256): 261638848512,
    ("g7_cfg1_2x_c48", 540, 960): 2063869839360,
}


@pytest.mark.parametrize("model,H,W", list(PARENT_FLOPS))
def test_flops_are_the_sum_over_the_steps_and_unchanged(model, H, W):
    cfg = bench.MODELS[model] if model in bench.MODELS else GoldenCase(model).config
    h = _ffi.Handle(cfg, BF16)
    flops = h.flops_per_image(H, W)
    h.close()
    assert flops == PARENT_FLOPS[(model, H, W)] and float(flops).is_integer()
    for _, (m, _, h_, w_, _) in bench.WORKLOADS.items():
        assert (m, h_, w_) in PARENT_FLOPS


# ---- knobs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g3_4x_c16", "g7_cfg1_2x_c48", "4x96"])
def test_no_fuse_gives_every_block_a_mix_and_a_z(name, monkeypatch):
    cfg = bench.MODELS[name] if name in bench.MODELS else GoldenCase(name).config

    def blocks(env):
        """(channels, fused, the conv2's output, the step after it) of every block, under `env`."""
        set_knobs(monkeypatch, env)
        h = _ffi.Handle(cfg, BF16)  # reads the knobs
        steps = check_schedule(h, cfg, BF16, 1, 37, 45, True)
        h.close()
        return [(s["cout"], s["fused"], s["off"][2], steps[i + 1]) for i, s in enumerate(steps) if s["op"] == CONV2]

    unfused, default = blocks({"MZ_NO_FUSE": "1"}), blocks({})
    layers = sum(cfg[f"{n}_layers"] for n in ("primary", "secondary", "tertiary", "quaternary"))
    assert len(unfused) == len(default) == layers + {2: 1, 4: 2, 8: 3}[cfg["upscale_ratio"]]
    for c, fused, z, nxt in unfused:  # conv2 into z, then the mix of the block input and z
        assert not fused and nxt["kind"] == MIX and nxt["cout"] == c and nxt["off"][1] == z and nxt["off"][2] != z
    for (c, fused, out, nxt), (_, _, z, _) in zip(default, unfused):
        assert fused == (c <= 96)
        if fused:  # neither: the block's result straight from conv2, nothing in z
            assert nxt["kind"] != MIX and out != z
        else:
            assert nxt["kind"] == MIX and out == z
