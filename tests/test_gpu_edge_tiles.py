"""GPU tests of the edge-class pixel tiles of the int16 3x3 conv (k_conv_i16<3, 1, 3|4, NST, 1, true>): the same bits with the
feature on (default) and off (option no_edge_tiles), against the compiled reference's fixture, the oracle and the known-answer
layers; and the batch-64 plan runs them where they apply."""
import importlib.util
import os

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
KAT = np.load(os.path.join(ROOT, "tests", "golden", "kat_layers.npz"))
FULL = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))


def _qsets():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.Q_SETS


@pytest.fixture(scope="module", autouse=True)
def driver():
    L = hipdrv.lib()
    assert L.yolo2_hip_device_count() >= 1, "no GPU visible: these tests must run on the GPU box"
    hipdrv.check(L.yolo2_accel_init(), "yolo2_accel_init")
    yield L
    L.yolo2_accel_cleanup()


def _process_option(name, value):
    hipdrv.check(hipdrv.lib().yolo2_hip_set_option(None, name.encode(), None if value is None else str(value).encode()),
                 "yolo2_hip_set_option")


def _edge_layers(ctx):
    return [l.idx for l in net.CONVS if "edge=1" in ctx.conv_plan(l.ord)]


@pytest.mark.parametrize("qset", ["std", "varq"])
def test_fullnet_edge_tiles_on_off_bit_identical(qset):
    """Batches 1, 3, 21, 22 and 64 (three lanes), feature on and off: frame 0 equals the reference fixture, and every frame is
    identical across the two settings."""
    model = synth.SynthModel(seed=int(FULL["meta/model_seed"]), **_qsets()[qset])
    fseed = int(FULL["meta/frame_seed"])
    frames = np.concatenate([synth.frames(fseed, 1), synth.frames(fseed + 1, 63)])
    want0 = FULL[f"i16/{qset}/region_raw_i16"].reshape(425, 13, 13)
    out = {}
    for off in (0, 1):
        ctx = hipdrv.Yolo2Hip(0)
        if off:
            ctx.set_option("no_edge_tiles", 1)
        ctx.load_model(model)
        for batch in (1, 3, 21, 22, 64):
            region, q = ctx.run_batch_host(frames[:batch])
            assert q == int(FULL[f"i16/{qset}/final_q"])
            assert np.array_equal(region[0], want0), (qset, off, batch)
            edge = _edge_layers(ctx)
            assert (not edge) if off else (batch < 21 or edge), (qset, off, batch, edge)
            out[off, batch] = region.copy()
        ctx.close()
    for batch in (1, 3, 21, 22, 64):
        assert np.array_equal(out[0, batch], out[1, batch]), batch


def test_fullnet_edge_tiles_random_q_table_vs_oracle():
    """A random per-layer Q table (forms C and D next to others): batches 3 and 22 with edge-class tiles equal the oracle."""
    rng = np.random.default_rng(31)
    wq = [int(v) for v in rng.integers(12, 16, 23)]
    bq = [int(v) for v in rng.integers(8, 15, 23)]
    aq = [14] + [int(v) for v in rng.integers(7, 12, 23)]
    model = synth.SynthModel(seed=31, weight_q=wq, bias_q=bq, act_q=aq, gain=1.0)
    frames = synth.frames(231, 22)
    orclib.oracle().orc_set_threads(16)
    check = (0, 1, 2, 21)
    want = {f: orclib.forward_i16(model, frames[f])[0] for f in check}
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(model)
    for batch in (3, 22):
        region, q = ctx.run_batch_host(frames[:batch])
        assert q == aq[23]
        assert _edge_layers(ctx), batch
        for f in check:
            if f < batch:
                assert np.array_equal(region[f].reshape(-1), want[f]), (batch, f)
    ctx.close()


KAT_3X3 = [str(n) for n in KAT["conv_i16/names"] if int(KAT[f"conv_i16/{n}/params"][2]) == 3 and int(KAT[f"conv_i16/{n}/params"][3]) == 1]


def _driver_p(C, N, W, H):
    """Pixels per lane plan_conv gives a form C / D call of the driver tier (one frame): the first of 8, 4, 2, 1 whose grid has
    at least 1024 workgroups, else 1."""
    P = 8
    while P > 1 and -(-W * H // (64 * P)) * -(-N // 32) < 1024:
        P //= 2
    return P


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("path", [None, 3, 4])
@pytest.mark.parametrize("name", KAT_3X3)
def test_conv_i16_kat_edge_tiles_on_off(name, path, off, driver):
    """Every 3x3 known-answer conv (saturating chains, 32-bit overflow corners, ragged 17 x 19, 5 x 5, 52 x 52) through the driver
    tier with edge-class tiles forced on and off, in the forms that can run them (C, D, and the loader's own choice): the known
    answer either way, and the edge kernel ran exactly when it applies."""
    _process_option("force_path", path)
    _process_option("no_edge_tiles", off)
    try:
        C, N, K, stride, W, H, pad, leaky, Qw, Qai, Qao, Qb = (int(v) for v in KAT[f"conv_i16/{name}/params"])
        x, wr, b, y = (KAT[f"conv_i16/{name}/{k}"] for k in ("x", "w_reorg", "bias", "y"))
        got = hipdrv.conv_layer_i16(x, wr, b, C, N, K, stride, W, H, pad, leaky, Qw, Qai, Qao, Qb, fill=0)
        assert np.array_equal(got, y), f"{name}: {int((got != y).sum())} of {y.size} differ"
        form = driver.yolo2_hip_last_layer_path()
        want_edge = not off and form in (3, 4) and H >= 3 and W >= 3 and _driver_p(C, N, W, H) == 1
        assert driver.yolo2_hip_last_layer_edge() == int(want_edge), (name, path, off, form)
    finally:
        _process_option("force_path", None)
        _process_option("no_edge_tiles", None)


@pytest.mark.parametrize("path", [None, 3])
def test_conv_i16_edge_tiles_wide_map_vs_oracle(path, driver):
    """A 400-pixel-wide map: interior runs of 868 items (the NST = 8 instantiation) and 803-item row patches, forms D (the
    loader's choice for these weights) and C, saturating both ways, against the oracle."""
    _process_option("force_path", path)
    try:
        rng = np.random.default_rng(77)
        C, N, W, H = 8, 40, 400, 5
        Qai, Qao, s_shift = 9, 9, 14
        Qw = s_shift + Qao - Qai
        wmax = min(32767 >> (16 - s_shift), (1 << s_shift) // 5)
        x = np.zeros((C, H, orclib.w8(W)), dtype=np.int16)
        x[:, :, :W] = rng.integers(-32768, 32768, (C, H, W))
        w = rng.integers(-wmax, wmax + 1, (N, C, 3, 3)).astype(np.int16)
        b = rng.integers(-32767, 32768, N).astype(np.int16)
        wr = synth.reorg_weights(w, C, N, 3)
        want = orclib.conv_i16(x, wr, b, C, N, 3, 1, W, H, 1, 1, Qw, Qai, Qao, 9)
        got = hipdrv.conv_layer_i16(x, wr, b, C, N, 3, 1, W, H, 1, 1, Qw, Qai, Qao, 9)
        assert driver.yolo2_hip_last_layer_path() == (4 if path is None else 3)
        assert driver.yolo2_hip_last_layer_edge() == 1
        assert np.array_equal(got, want)
        assert (want == 32767).any() and (want <= -3276).any()
    finally:
        _process_option("force_path", None)


def test_batch64_plan_runs_edge_tiles_on_layers_8_to_29():
    """At batch 64 every 3x3 conv of layers 8..29 that is not fused with its pool runs edge-class tiles (and no 1x1 conv or fused
    layer does); the option turns them all off without changing the plan source."""
    model = synth.SynthModel(seed=1)
    frames = synth.frames(5, 64)
    srcs = {}
    for off in (0, 1):
        ctx = hipdrv.Yolo2Hip(0)
        if off:
            ctx.set_option("no_edge_tiles", 1)
        ctx.load_model(model)
        ctx.run_batch_host(frames)
        srcs[off] = ctx.plan_source()
        for l in net.CONVS:
            plan = ctx.conv_plan(l.ord)
            if l.size == 1 or 8 <= l.idx <= 29:
                want = not off and l.size == 3 and "fused=0" in plan
                assert ("edge=1" in plan) == want, (off, l.idx, plan)
        if not off:
            assert {8, 12, 14, 16, 18, 20, 22, 23, 24, 29} <= set(_edge_layers(ctx))
        ctx.close()
    assert srcs[0] == srcs[1]
