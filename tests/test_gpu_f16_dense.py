"""Per-launch parity of the fp16 and split-fp16 passes on full-mantissa fp32 weights (tests/f16models.py), on the MI355X.

synth.SynthModel's weights are int16 values times 2^-14: the w_lo block at the tail of the split pass's packed weights [w_hi | w_hi |
w_lo] is all zero on the nine 3x3 layers from 12 on, so a kernel that stopped its contraction after two parts, read w_lo at a wrong
offset, or a packer that wrote a wrong lo would pass every test that loads them.  DenseModel fills the mantissa: > 97 % of the weights
have w_lo != 0, most of them fp16 subnormals, so these tests also rest on the packer producing subnormals and the MFMA keeping them.

The batch is 2 (the smallest with a ragged last 256-pixel tile): frame 0 = synth.frames(40, 1), frame 1 = the dog letterbox, which is
the frame judged.  The judge is tests/f16ref.py's per-launch checker, unchanged; YOLO2_F16_PARITY_LOG=<file> collects the lines."""
import os

import numpy as np
import pytest

import f16models as fm
import f16ref as fr
import orclib
from test_gpu_f16_layers import SPLIT_VARIANTS, check_frame, kernels, log, read, run
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
B, JUDGED = 2, 1


def dog_letterbox():
    return hipdrv.letterbox_u8(np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"])[None]


@pytest.fixture(scope="module")
def frames():
    return np.concatenate([synth.frames(40, 1), dog_letterbox()])


@pytest.fixture(scope="module")
def dense():
    """(spread) -> (model, fr.Weights), built once."""
    made, base = {}, synth.SynthModel(seed=1)

    def get(spread):
        if spread not in made:
            m = fm.DenseModel(1, spread, base=base)
            made[spread] = (m, fr.Weights(m))
        return made[spread]
    return get


@pytest.fixture(scope="module")
def default_runs(dense, frames):
    """(split, spread) -> (ctx, region) of the default plan at batch 2, run once and shared; closed when the module is done."""
    made = {}

    def get(split, spread):
        if (split, spread) not in made:
            made[(split, spread)] = run(dense(spread)[0], frames, split)
        return made[(split, spread)]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def tag(split, spread, what="dense"):
    return f"{what}-{'split' if split else 'fp16'}-s{spread}"


@pytest.mark.parametrize("split,spread", [(False, 0.5), (True, 0.5), (True, 3.0)], ids=["fp16-0.5", "split-0.5", "split-3.0"])
def test_dense_default_plan_every_launch(split, spread, dense, default_runs, frames):
    """Default plan, dense weights: every launch of the letterbox frame inside its hard bound and statistical limits, and every tensor
    finite with max |v| < 2^12 (far from fp16 overflow: a failure is never an overflow artefact)."""
    W = dense(spread)[1]
    ctx, region = default_runs(split, spread)
    table = kernels(ctx, split)
    log(f"== {tag(split, spread)} B={B}: " + " ".join(f"L{k}:{v}" for k, v in sorted(table.items())))
    vmax = {}
    for L in sorted(table):
        last = fr.step_layers(table, L)[-1]
        for f in range(B):
            v = region[f].astype(np.float64) if last == 30 else read(ctx, last, f, split)[0]["v"]
            assert np.isfinite(v).all(), (L, f)
            vmax[last] = max(vmax.get(last, 0.0), float(np.abs(v).max()))
    log(f"{tag(split, spread)} max |v| per written tensor: " + " ".join(f"L{k}:{v:.3g}" for k, v in sorted(vmax.items())))
    assert max(vmax.values()) < 2.0 ** 12, vmax
    bad = check_frame(ctx, split, JUDGED, B, frames, region, W, tag(split, spread))
    assert not bad, bad


@pytest.mark.parametrize("name", SPLIT_VARIANTS)
def test_dense_split_variants_changed_launches(name, dense, default_runs, frames, monkeypatch):
    """The alternative split kernels keep the w_lo block at a place of their own: every launch whose kernel differs from the default
    plan's, dense weights, spread 0.5.  (The fp16 variants are not repeated: after packing the fp16 kernels see the same kind of data
    as with the grid weights.)"""
    model, W = dense(0.5)
    base = kernels(default_runs(True, 0.5)[0], True)
    ctx, region = run(model, frames, True, {name: "1"}, monkeypatch)
    table = kernels(ctx, True)
    changed = {L for L in table if base.get(L) != table[L]}
    log(f"== dense variant {name} (split): " + " ".join(f"L{L}:{table[L]}" for L in sorted(changed)))
    assert changed, "the toggle did not change the launch table"
    bad = check_frame(ctx, True, JUDGED, B, frames, region, W, "dense-" + name.replace("YOLO2_F16_", "") + "-split", only=changed)
    ctx.close()
    assert not bad, bad


def test_dropped_w_lo_is_rejected_on_gpu_data(dense, default_runs, frames):
    """On real GPU data (split default plan, spread 0.5): the launches at layers 2, 12, 22, 29 and 30 pass, and the same launches
    against a reference without a_hi * w_lo are rejected - the term the grid weights leave at zero from layer 12 on."""
    W = dense(0.5)[1]
    ctx, region = default_runs(True, 0.5)
    only = {2, 12, 22, 29, 30}
    assert only <= set(kernels(ctx, True))
    assert not check_frame(ctx, True, JUDGED, B, frames, region, W, "no_wlo-ok", only=only)
    bad = check_frame(ctx, True, JUDGED, B, frames, region, W, "no_wlo", only=only, mutate=("no_wlo",))
    assert set(bad) == only, f"a dropped a_hi * w_lo was accepted at layers {sorted(only - set(bad))}"


def _boxes(region_f32):
    """All 845 cell / anchor slots decoded without a threshold or NMS: rows in slot order."""
    proc = np.zeros(425 * 169, dtype=np.float32)
    orclib.host().y2h_region_forward(np.ascontiguousarray(region_f32.reshape(-1), dtype=np.float32), proc)
    rows = np.zeros((845, 85), dtype=np.float32)
    orclib.host().y2h_boxes_nms(proc, 640, 480, 0.0, 0.0, rows, 845)
    return rows[rows[:, 4] > 0]


# regression guards of test_dense_f32tol_every_box_within_1e_3: 8 x the worst error measured on the MI355X, rounded up to one
# significant digit (coordinates capped at the contract's 1e-3).  Measured (profiles/r07_f16_dense_parity.txt): worst coordinate
# error 2.26e-5 -> 8 x = 1.81e-4 -> 2e-4; worst objectness error 4.98e-6 -> 8 x = 3.98e-5 -> 4e-5.
COORD_GUARD = 2e-4
OBJ_GUARD = 4e-5


def test_dense_f32tol_every_box_within_1e_3(dense):
    """The project's contract (BASELINE.json: detections within 1e-3 box-coordinate tolerance for fp32) on dense weights, spread 0.5,
    ragged batch 3 (two synthetic frames + the dog letterbox), against the fp32 oracle run on the same DenseModel: raw region tensor
    within 1e-3 absolute, all four coordinates of all 845 slots within 1e-3.  Measured on the MI355X: raw 3.29e-5 on values up to
    5.58, coordinates 2.26e-5, objectness 4.98e-6; the regression guards are 8 x those (COORD_GUARD 2e-4, OBJ_GUARD 4e-5), so a fall
    back to fp16-like accuracy (5.8e-3 on the grid weights) cannot pass by luck."""
    model = dense(0.5)[0]
    frames = np.concatenate([synth.frames(40, 2), dog_letterbox()])
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    region = ctx.run_batch_f32tol_host(frames)
    ctx.close()
    orclib.oracle().orc_set_threads(16)
    worst = {"raw": 0.0, "coord": 0.0, "obj": 0.0, "max |v|": 0.0}
    for k in range(3):
        ref = orclib.forward_f32(model, frames[k]).reshape(425, 13, 13)
        ra, ga = _boxes(ref), _boxes(region[k])
        assert len(ra) == len(ga) == 845
        worst["raw"] = max(worst["raw"], float(np.abs(region[k] - ref).max()))
        worst["coord"] = max(worst["coord"], float(np.abs(ga[:, :4] - ra[:, :4]).max()))
        worst["obj"] = max(worst["obj"], float(np.abs(ga[:, 4] - ra[:, 4]).max()))
        worst["max |v|"] = max(worst["max |v|"], float(np.abs(ref).max()))
    log("dense f32tol worst errors (spread 0.5, B=3, vs the fp32 oracle): " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst["raw"] <= 1e-3, worst
    assert worst["coord"] <= 1e-3, worst
    assert worst["coord"] <= COORD_GUARD and worst["obj"] <= OBJ_GUARD, worst
