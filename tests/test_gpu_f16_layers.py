"""Per-launch parity of the fp16 and split-fp16 passes against an fp64 reference (tests/f16ref.py), on the MI355X.

Every launch of the launch table is judged alone: its input is the GPU's own tensor read back raw (yolo2_hip_debug_f16_tensor), its
output is compared with the fp64 reference of the same arithmetic under a hard per-element bound and per-partition statistics in
output ulps.  These tests are the gate for any change to csrc/kernels_f16.hpp, hipcc or the compile flags.  Each step prints one line
(kernel, max |err| in units, worst ratio to the hard bound, statistics border vs interior); YOLO2_F16_PARITY_LOG=<file> appends them
to a file as well."""
import os

import numpy as np
import pytest

import f16ref as fr
import orclib
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT

# the YOLO2_F16_* kernel variants (every f16_* option but the diagnostic ones: tests/test_f16_layer_ref.py checks the list is complete)
F16_VARIANTS = ["YOLO2_F16_NO_HALO", "YOLO2_F16_NO_WIDE", "YOLO2_F16_NO_MFMA0", "YOLO2_F16_NO_GLDS", "YOLO2_F16_NO_POOLFUSE", "YOLO2_F16_W8",
                "YOLO2_F16_NO_PERSIST", "YOLO2_F16_PERSIST_ALL", "YOLO2_F16_M16", "YOLO2_F16_RING_ALL", "YOLO2_F16_NO_RING", "YOLO2_F16_NO_C32",
                "YOLO2_F16_NO_RW", "YOLO2_F16_NO_RWB", "YOLO2_F16_NO_RWC", "YOLO2_F16_NO_FUSE1X1", "YOLO2_F16_RING256", "YOLO2_F16_RING_SQ"]
# variants whose switch selects a kernel the default plan does not run anyway (the default takes layers 2 / 4 / 6 with rwc / rwb, so
# the c32 and persistent-halo kernels they would disable are not in it): the table stays as it is
F16_VARIANTS_SAME_TABLE = {"YOLO2_F16_NO_PERSIST", "YOLO2_F16_NO_C32"}
SPLIT_VARIANTS = ["YOLO2_F16_NO_MFMA0", "YOLO2_F16_NO_HALO"]
KLEAD, KTAIL = 64, 1024   # csrc/layout.hpp


@pytest.fixture(scope="module")
def model():
    return synth.SynthModel(seed=1)


@pytest.fixture(scope="module")
def weights(model):
    return fr.Weights(model)


def ragged_frames():
    """Batch 5: four synthetic frames + the letterbox of dog.npz last (its flat grey border gives exact zeros and negatives)."""
    dog = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))
    return np.concatenate([synth.frames(40, 4), hipdrv.letterbox_u8(dog["rgb"])[None]])


def log(line):
    print(line)
    p = os.environ.get("YOLO2_F16_PARITY_LOG")
    if p:
        with open(p, "a") as f:
            f.write(line + "\n")


def kernels(ctx, split):
    if split:
        return {i: k for i in range(32) if (k := ctx.f32tol_layer_kernel(i))}
    return ctx.fp16_layer_kernels()


def read(ctx, layer, frame, split):
    raw, g = ctx.debug_f16_tensor(layer, frame, split)
    return fr.decode(raw, g, split), raw, g


def step_input(ctx, L, frame, split, frames):
    if L == 0:
        return dict(v=frames[frame].astype(np.float64))
    if L == 29:   # the concat tensor: channels 0..255 = reorg (layer 27), 256.. = layer 24
        a, b = read(ctx, 27, frame, split)[0], read(ctx, 24, frame, split)[0]
        return {k: np.concatenate([a[k], b[k]]) for k in ("v", "hi", "lo")}
    return read(ctx, fr.input_layer(L), frame, split)[0]


def check_frame(ctx, split, frame, B, frames, region, W, tag, only=None, mutate=None):
    """Checks every launch (or those whose first layer is in `only`) of the last run for one frame; returns {layer: failures}."""
    path = "split" if split else "fp16"
    table = kernels(ctx, split)
    bad = {}
    for L in sorted(table):
        if only is not None and L not in only:
            continue
        kernel = table[L]
        layers = fr.step_layers(table, L)
        x = step_input(ctx, L, frame, split, frames)
        res = fr.step_ref(path, kernel, layers, x, W, mutate=mutate)
        last = layers[-1]
        if last == 30:
            gpu = region[frame].astype(np.float64)
        else:
            gpu = read(ctx, last, frame, split)[0]["v"]
        C, H, Wd = gpu.shape
        tail = None
        if frame == B - 1 and (B * H * Wd) % 256:
            first = (B * H * Wd) // 256 * 256 - frame * H * Wd
            tail = np.arange(max(first, 0), H * Wd)
        fails, rep = fr.check_step(gpu, res, tail=tail)
        log(fr.report_line(f"{tag} f{frame} L{L}", kernel, rep) + ("" if not fails else "  FAIL: " + fails[0]))
        if fails:
            bad[L] = fails
    return bad


def run(model, frames, split, env=None, monkeypatch=None):
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    region = ctx.run_batch_f32tol_host(frames) if split else ctx.run_batch_fp16_host(frames)
    if env:
        for k in env:
            monkeypatch.delenv(k)
    return ctx, region


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_default_plan_every_launch(split, model, weights):
    """Default plan of both passes, ragged batch 5 (dog letterbox last): every launch of frames 0 and 4 inside its bound and limits."""
    frames = ragged_frames()
    ctx, region = run(model, frames, split)
    table = kernels(ctx, split)
    log(f"== default {'split' if split else 'fp16'} B=5: " + " ".join(f"L{k}:{v}" for k, v in sorted(table.items())))
    bad = {}
    for f in (0, 4):
        bad.update({(f, L): v for L, v in check_frame(ctx, split, f, 5, frames, region, weights, "default" + ("-split" if split else "")).items()})
    ctx.close()
    assert not bad, bad


@pytest.mark.parametrize("env", F16_VARIANTS + [("split", e) for e in SPLIT_VARIANTS],
                         ids=lambda e: e if isinstance(e, str) else "split-" + e[1])
def test_variant_every_changed_launch(env, model, weights, monkeypatch):
    """Every YOLO2_F16_* variant (and the split pass's): the toggle changes the launch table where it should, and every launch whose
    kernel differs from the default plan's is checked on frame 4 of the ragged batch (the kernels they share with the default plan
    are checked by test_default_plan_every_launch)."""
    split = not isinstance(env, str)
    name = env[1] if split else env
    frames = ragged_frames()
    ctx0, _ = run(model, frames[:1], split)
    base = kernels(ctx0, split)
    ctx0.close()
    ctx, region = run(model, frames, split, {name: "1"}, monkeypatch)
    table = kernels(ctx, split)
    changed = {L for L in table if base.get(L) != table[L]}
    log(f"== variant {name}{' (split)' if split else ''}: " + " ".join(f"L{L}:{table[L]}" for L in sorted(changed)))
    if name in F16_VARIANTS_SAME_TABLE and not split:
        assert table == base, "the toggle changed the table"
    else:
        assert table != base, "the toggle did not change the launch table"
    bad = check_frame(ctx, split, 4, 5, frames, region, weights, name.replace("YOLO2_F16_", "") + ("-split" if split else ""), only=changed)
    ctx.close()
    assert not bad, bad


def test_lanes_and_run_walking_batch130(model, weights):
    """Batch 130 = two lanes of 65 (k_conv_f16_rwc walks runs of 26 row pairs, more runs than workgroups): frames 0, 64 (last of lane 0),
    65 (first of lane 1) and 129, every launch."""
    frames = np.concatenate([synth.frames(310 + k, 1) for k in range(4)] * 33)[:130]
    ctx, region = run(model, frames, False)
    assert ctx.num_lanes_fp16() == 2
    table = kernels(ctx, False)
    assert table[2] == "k_conv_f16_rwc" and table[6] == "k_conv_f16_rwb<pool>"
    bad = {}
    for f in (0, 64, 65, 129):
        bad.update({(f, L): v for L, v in check_frame(ctx, False, f, 65, frames, region, weights, "B130").items()})
    ctx.close()
    assert not bad, bad


# the size guards of build_f16_plan (csrc/yolo2_fp16.hip), restated: smallest batch past each
def _pl(hw):
    return (hw + 1) * (hw + 1)


def _first_past(pred):
    b = 1
    while pred(b):
        b += 1
    return b


GUARDS = {
    # split layer 4: halo_p needs (kLead + B PL) max(Cp_in, Cp_out) 2 < 2^32 (off32); 64 / 128 channels -> 192 / 384-half split items
    "split-L4-halo_p": (True, 4, _first_past(lambda B: (KLEAD + B * _pl(104)) * max(192, 384) * 2 < 2 ** 32),
                        lambda k: k.startswith("k_conv_f16_halo_p")),
    # fp16 layer 2: rwc needs (kLead + B PL + kTail) 64 < 2^31
    "fp16-L2-rwc": (False, 2, _first_past(lambda B: (KLEAD + B * _pl(208) + KTAIL) * 64 < 2 ** 31), lambda k: k == "k_conv_f16_rwc"),
    # fp16 layers 4 / 6: rw* needs (kLead + B PL + kTail) 128 < 2^31
    "fp16-L4-rw": (False, 4, _first_past(lambda B: (KLEAD + B * _pl(104) + KTAIL) * 128 < 2 ** 31), lambda k: k.startswith("k_conv_f16_rw")),
}


@pytest.mark.parametrize("guard", list(GUARDS))
def test_size_guard_flips_kernel_and_last_frame_is_right(guard, model, weights, monkeypatch):
    """With YOLO2_F16_NO_LANES=1, the smallest batch past each 32-bit offset guard of build_f16_plan: the table flips between B - 1 and
    B, and every launch of the LAST frame, whose items lie beyond 2^31 / 2^32 bytes, is inside its bound.  Frames of period 4.
    Memory: split B = 508: ~1 GB of host frames, ~50 GB of split activations; fp16 B = 769 / 1522: 1.6 / 3.2 GB of host frames,
    ~10 / ~20 GB of activations."""
    split, layer, B, is_guarded = GUARDS[guard]
    assert B in (508, 769, 1522), B        # (today's code: a change of these numbers means the guards moved - update the docstring)
    base = np.concatenate([synth.frames(300 + k, 1) for k in range(4)])
    frames = np.concatenate([base] * ((B + 3) // 4))[:B]
    monkeypatch.setenv("YOLO2_F16_NO_LANES", "1")
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    rb = ctx.run_batch_f32tol_host if split else ctx.run_batch_fp16_host
    rb(frames[:B - 1])
    before = kernels(ctx, split)
    region = rb(frames)
    after = kernels(ctx, split)
    log(f"== guard {guard}: B={B - 1} L{layer} {before[layer]} -> B={B} L{layer} {after[layer]}")
    assert is_guarded(before[layer]) and not is_guarded(after[layer]), (before[layer], after[layer])
    bad = check_frame(ctx, split, B - 1, B, frames, region, weights, f"guard {guard}")
    assert np.array_equal(region[B - 1], region[(B - 1) % 4]), "the last frame differs from the same frame at the front of the batch"
    ctx.close()
    assert not bad, bad


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_padding_stays_zero_and_unwritten_tensors_are_refused(split, model):
    """After two consecutive runs with different frames: every written tensor's pad row and column, the channels beyond C (split: each
    part's tail and the [3 part_stride, Cp) tail) and the lead / tail items are exact zeros.  Tensors the plan does not write are
    refused with a clear error."""
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    rb = ctx.run_batch_f32tol_host if split else ctx.run_batch_fp16_host
    rb(synth.frames(50, 3))
    rb(ragged_frames()[2:5])
    table = kernels(ctx, split)
    n_checked = 0
    for L in range(31):
        l = net.LAYERS[L]
        if l.type in (net.ROUTE, net.REGION) or L == 30:
            continue
        written = any(L == fr.step_layers(table, s)[-1] for s in table)
        if not written:
            with pytest.raises(hipdrv.Yolo2HipError, match="not written by the current fp16 plan|has no tensor"):
                ctx.debug_f16_tensor(L, 0, split)
            continue
        for f in range(3):
            raw, g = ctx.debug_f16_tensor(L, f, split)
            assert fr.padding_violations(raw, g, split) == [], (L, f)
        for which in (1, 2):
            raw, g = ctx.debug_f16_tensor(L, 2, split, which)
            assert raw.shape[0] == (KLEAD if which == 1 else KTAIL) and not raw.any(), (L, which)
        n_checked += 1
    assert n_checked >= 15, n_checked
    with pytest.raises(hipdrv.Yolo2HipError, match="region tensor"):
        ctx.debug_f16_tensor(30, 0, split)
    with pytest.raises(hipdrv.Yolo2HipError, match="not written"):
        ctx.debug_f16_tensor(0, 0, split)
    if not split:   # fused pool (rwc), the 128-channel tensor inside rwb<+1x1>, layer 8 inside halo+1x1
        assert table[2] == "k_conv_f16_rwc" and table[4] == "k_conv_f16_rwb<+1x1>" and table[8] == "k_conv_f16_halo<256,2,16>+1x1"
        for L in (2, 4, 8):
            with pytest.raises(hipdrv.Yolo2HipError, match="not written"):
                ctx.debug_f16_tensor(L, 0, split)
    with pytest.raises(hipdrv.Yolo2HipError, match="outside the last batch"):
        ctx.debug_f16_tensor(11, 3, split)
    ctx.close()


@pytest.mark.parametrize("layer,mut", [(2, ("drop_border_tap", 7)), (6, ("pool_offset",)), (8, ("no_bias_block", 2)), (29, ("drop_channel", 300)),
                                       (29, ("rtz",)), (6, ("leaky", 0.125)), (8, ("shift_tile", 512))])
def test_checker_has_teeth_on_gpu_data(layer, mut, model, weights):
    """On real GPU data (default fp16 plan, batch 5, frame 0): the launches of layers 2 (rwc), 6 (rwb<pool>), 8 (halo+1x1) and 29 (input
    = the concat tensor) pass, and a reference with one deliberate error is rejected."""
    frames = ragged_frames()
    ctx, region = run(model, frames, False)
    assert not check_frame(ctx, False, 0, 5, frames, region, weights, "teeth-ok", only={layer})
    bad = check_frame(ctx, False, 0, 5, frames, region, weights, f"teeth {mut[0]}", only={layer}, mutate=mut)
    ctx.close()
    assert layer in bad, f"mutation {mut} at layer {layer} was accepted"
