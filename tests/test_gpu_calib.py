"""GPU tests of the calibration tier (include/yolo2_hip.h "calibration"): the abs-max reduction against numpy, the quantiser against
the oracle's input-quantise rule, the statistics of the exact fp32 pass against the oracle's fp32 layer dumps (bit for bit), the Q
tables against the rule restated here in double, and the calibrated int16 weight set running bit-exactly like the oracle on it -
closer to fp32 than the hand-picked STD_Q tables - for SynthModel and for the full-mantissa DenseModel, which had no int16 form.

The CPU oracle costs seconds per frame: its results are computed once per module and shared."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import f16models
import orclib
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu
NCONV = len(net.CONVS)
ORD24 = next(l.ord for l in net.CONVS if l.idx == 24)
ORD26 = next(l.ord for l in net.CONVS if l.idx == 26)
WOFF = np.concatenate([[0], np.cumsum(net.WEIGHT_LEN)])
BOFF = np.concatenate([[0], np.cumsum(net.BIAS_LEN)])
PKG = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")


def q_rule(m, h=1.0):
    """the rule, in double: the largest q in 0..15 at which h m 2^q still rounds (half away from zero) to at most 32767"""
    m = float(m)
    if m == 0.0:
        return 15
    for q in range(15, -1, -1):
        if h * m * 2.0 ** q < 32767.5:
            return q
    raise AssertionError(f"no q holds {m}")


def tables_by_rule(act, w, b, headroom=1.0):
    wq = [q_rule(m) for m in w]
    bq = [q_rule(m) for m in b]
    aq = [q_rule(act[0])] + [q_rule(m, headroom) for m in act[1:]]
    if aq[ORD24 + 1] > aq[ORD26 + 1]:
        aq[ORD24 + 1] = aq[ORD26 + 1]
    return wq, bq, aq


def layer_maxima(blob, offs):
    return np.array([np.abs(blob[offs[o]:offs[o + 1]]).max() for o in range(NCONV)], dtype=np.float32)


def saturated(a):
    return int(((a == 32767) | (a == -32768)).sum())


def oracle_i16(model, frame, dump=False):
    orclib.oracle().orc_set_threads(min(16, os.cpu_count() or 1))
    return orclib.forward_i16(model, frame, dump=dump)


# ------------------------------------------------------------------ shared, computed once

@pytest.fixture(scope="module")
def model():
    return synth.SynthModel(seed=1, obj_bias=2.0)


@pytest.fixture(scope="module")
def frames():
    return synth.frames(1, 2)


@pytest.fixture(scope="module")
def oracle_stats(model, frames):
    """max |.| of the oracle's fp32 layer dumps on frame 0: [24] (the frame, then every conv output), and its region tensor"""
    orc = orclib.oracle()
    orc.orc_set_threads(min(16, os.cpu_count() or 1))
    w, b = model.weights_f32(), model.bias_f32()
    wp = orclib.OrcWeightsF32(w.ctypes.data, b.ctypes.data)
    region = np.zeros(425 * 169, dtype=np.float32)
    frame = np.ascontiguousarray(frames[0])
    dumps = (C.c_void_p * 32)()
    assert orc.orc_yolov2_forward_f32(C.byref(wp), frame.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p), dumps) == 0
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    act = [np.abs(frame).max()]
    for l in net.LAYERS:
        if not dumps[l.idx]:
            continue
        if l.type == net.CONV:
            n = l.out_c * l.out_h * orclib.w8(l.out_w)
            t = np.ctypeslib.as_array(C.cast(dumps[l.idx], C.POINTER(C.c_float)), shape=(n,)).reshape(l.out_c, l.out_h, orclib.w8(l.out_w))
            act.append(np.abs(t[:, :, :l.out_w]).max())
        libc.free(dumps[l.idx])
    assert len(act) == NCONV + 1
    return np.array(act, dtype=np.float32), region


@pytest.fixture(scope="module")
def ctx(model):
    """a context holding the model's fp32 twin"""
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    yield c
    c.close()


@pytest.fixture(scope="module")
def calibrated(ctx, frames):
    """the model calibrated on frame 0 (headroom 1)"""
    return ctx.calibrate(frames=frames[:1], batch=1)


@pytest.fixture(scope="module")
def calibrated_run(calibrated, frames):
    """the calibrated set on the int16 pass, frames 0 and 1: (region [2], final Q, layer tensors of frame 0 the pass materialised)"""
    c = hipdrv.Yolo2Hip(0)
    c.load_model(calibrated)
    region, q = c.run_batch_host(frames)
    fused = c.pool_fused_layers()
    layers = {i: c.debug_layer_output(i, 0) for i in [-1] + [l.idx for l in net.LAYERS if l.type in (net.CONV, net.MAXPOOL)]
              if not (i in fused and i != 16)}
    c.close()
    return region, q, layers


# ------------------------------------------------------------------ 1. the reduction

SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 1027, 4 * 256 * 40 + 3]


def _absmax(x, offset_elems=0):
    """x (float32) in HBM at `offset_elems` floats behind a 256-byte-aligned allocation -> (max, non-finite count)"""
    buf = hipdrv.DevBuf(np.concatenate([np.full(offset_elems, 7e37, np.float32), x, np.full(5, 7e37, np.float32)]))   # neighbours that must not be read
    try:
        return hipdrv.absmax_f32(buf.addr + 4 * offset_elems, x.size)
    finally:
        buf.free()


@pytest.mark.parametrize("n", SIZES)
def test_absmax_equals_numpy(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    for where in sorted({0, n - 1, max(0, n - 2), n // 2}):      # first, last, a tail element (behind the last full float4), the middle
        for sign in (1.0, -1.0):
            y = x.copy()
            y[where] = sign * 37.25
            for off in (0, 1):                                    # 1: the range starts 4 bytes behind a 16-byte boundary
                m, bad = _absmax(y, off)
                assert (m, bad) == (np.float32(37.25), 0), (n, where, sign, off, m, bad)
    m, bad = _absmax(x, 3)
    assert m.tobytes() == np.abs(x).max().tobytes() and bad == 0


def test_absmax_zeros_subnormals_and_non_finite_values():
    n = 1027
    assert _absmax(np.zeros(n, np.float32)) == (0.0, 0)
    assert _absmax(np.full(n, -0.0, np.float32), 1) == (0.0, 0)
    x = np.zeros(n, np.float32)
    x[5], x[1025] = np.float32(3e-45), -np.float32(1e-40)          # subnormals: the larger one wins, bit for bit
    m, bad = _absmax(x)
    assert m.tobytes() == np.float32(1e-40).tobytes() and m > 0 and bad == 0
    x = np.random.default_rng(5).standard_normal(4 * 256 * 40 + 3).astype(np.float32)
    want = np.abs(x).max()
    y = x.copy()
    y[777], y[-1] = np.nan, -np.inf                                # counted, and not reported as the maximum
    m, bad = _absmax(y, 1)
    assert m.tobytes() == np.abs(np.delete(x, [777, x.size - 1])).max().tobytes() and bad == 2 and m <= want
    y = np.full(70, np.nan, np.float32)
    assert _absmax(y) == (0.0, 70)


# ------------------------------------------------------------------ 2. + 3. the quantiser

def _expected_i16(x, q):
    out = np.zeros(x.size, dtype=np.int16)
    orclib.oracle().orc_quantize_input(np.ascontiguousarray(x, dtype=np.float32), out, x.size, q)
    out[out == -32768] = -32767                                    # the clamp is symmetric here
    return out


def _crafted(n, q, seed):
    """n floats for Q = q: ties (k + 0.5) 2^-q of both signs, clear overflows, values in the last half step in front of the clamp,
    +-0, subnormals, random filler.  -> (values, number of overflows: |x 2^q| >= 32767.5)"""
    rng = np.random.default_rng(seed)
    s = 2.0 ** -q
    k = np.concatenate([np.arange(0, 40), [255, 256, 4095, 16383, 32765, 32766]]).astype(np.float64)
    ties = np.concatenate([(k + 0.5) * s, -(k + 0.5) * s])
    over = np.concatenate([[32767.5, 32768.0, 32768.5, 40000.0, 1e9], -np.array([32767.5, 32768.0, 32769.0, 65536.0, 1e12])]) * s
    edge = np.array([32767.0, 32767.25, 32767.49, -32767.0, -32767.25, 32766.5, -32766.5]) * s   # representable: not overflows
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 0.49999997 * s, -0.49999997 * s])
    special = np.concatenate([over, edge, tiny, ties]).astype(np.float32)[:3 * n // 4]     # (the 32 biases of layer 0 hold the first 24)
    x = (rng.standard_normal(n) * 8000 * s).astype(np.float32)
    x[rng.permutation(n)[:special.size]] = special
    n_over = int((np.abs(x.astype(np.float64) * 2.0 ** q) >= 32767.5).sum())       # (the filler's tail adds a few of its own)
    assert n_over >= over.size
    return x, n_over


def test_quantiser_equals_the_oracles_rule_on_crafted_values():
    """layers 0, 1 and 22 (the first, one in the middle of the streams, the last with its 425 biases) hold crafted values; every other
    layer is zero.  Bit-equal to orc_quantize_input with -32768 mapped to -32767; clamped = the crafted overflows."""
    w = np.zeros(hipdrv.N_WEIGHTS, np.float32)
    b = np.zeros(hipdrv.N_BIAS, np.float32)
    wq = np.full(NCONV, 14, np.int32)
    bq = np.full(NCONV, 12, np.int32)
    wq[[0, 1, 22]] = [14, 9, 15]
    bq[[0, 1, 22]] = [12, 0, 7]
    overflows = 0
    for o in (0, 1, 22):
        w[WOFF[o]:WOFF[o + 1]], k = _crafted(net.WEIGHT_LEN[o], int(wq[o]), 10 + o)
        overflows += k
        b[BOFF[o]:BOFF[o + 1]], k = _crafted(net.BIAS_LEN[o], int(bq[o]), 50 + o)
        overflows += k
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(w, b)
    wi, bi, clamped = c.quantize_weights(wq, bq)
    c.close()
    for o in range(NCONV):
        assert np.array_equal(wi[WOFF[o]:WOFF[o + 1]], _expected_i16(w[WOFF[o]:WOFF[o + 1]], int(wq[o]))), f"weights of conv {o}"
        assert np.array_equal(bi[BOFF[o]:BOFF[o + 1]], _expected_i16(b[BOFF[o]:BOFF[o + 1]], int(bq[o]))), f"biases of conv {o}"
    assert wi.min() == -32767 and wi.max() == 32767 and bi.min() == -32767
    assert clamped == overflows, (clamped, overflows)


def test_quantiser_round_trips_the_synthetic_model():
    """SynthModel's fp32 twin is int16 2^-Q: quantised with its own tables it is the int16 model again, byte for byte"""
    m = synth.SynthModel(seed=1)
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(m.weights_f32(), m.bias_f32())
    wi, bi, clamped = c.quantize_weights(m.weight_q, m.bias_q)
    c.close()
    assert wi.tobytes() == m.weights_i16().tobytes() and bi.tobytes() == m.bias_i16().tobytes()
    assert clamped == 0


# ------------------------------------------------------------------ 4. statistics

def test_statistics_equal_the_oracles_layer_maxima(ctx, model, frames, oracle_stats):
    want_act, want_region = oracle_stats
    ctx.calib_reset()
    assert ctx.calib_stats()["frames_seen"] == 0 and not ctx.calib_stats()["act_absmax"].any()
    ctx.calib_frames(frames[:1])
    st = ctx.calib_stats()
    assert st["frames_seen"] == 1
    assert st["act_absmax"].tobytes() == want_act.tobytes(), np.flatnonzero(st["act_absmax"] != want_act)
    assert st["act_absmax"][0] == np.abs(frames[0]).max()
    region = ctx.run_batch_fp32_host(frames[:1])
    assert np.array_equal(region.reshape(-1), want_region)
    assert st["act_absmax"][NCONV] == np.abs(region).max()
    assert st["weight_absmax"].tobytes() == layer_maxima(model.weights_f32(), WOFF).tobytes()
    assert st["bias_absmax"].tobytes() == layer_maxima(model.bias_f32(), BOFF).tobytes()
    # another frame only raises; the same two frames in one batch of 2 give the same statistics; reset clears
    ctx.calib_frames(frames[1:2])
    st2 = ctx.calib_stats()
    assert st2["frames_seen"] == 2 and (st2["act_absmax"] >= st["act_absmax"]).all() and (st2["act_absmax"] > st["act_absmax"]).any()
    assert np.array_equal(st2["weight_absmax"], st["weight_absmax"]) and np.array_equal(st2["bias_absmax"], st["bias_absmax"])
    ctx.calib_reset()
    st0 = ctx.calib_stats()
    assert st0["frames_seen"] == 0 and not st0["act_absmax"].any() and np.array_equal(st0["weight_absmax"], st["weight_absmax"])
    ctx.calib_frames(frames)
    st3 = ctx.calib_stats()
    assert st3["frames_seen"] == 2 and st3["act_absmax"].tobytes() == st2["act_absmax"].tobytes()
    assert st3["act_absmax"][NCONV] == np.abs(ctx.run_batch_fp32_host(frames)).max()


# ------------------------------------------------------------------ 5. tables

def test_tables_equal_the_rule_on_the_oracles_maxima(calibrated, model, oracle_stats):
    want_act, _ = oracle_stats
    wq, bq, aq = tables_by_rule(want_act, layer_maxima(model.weights_f32(), WOFF), layer_maxima(model.bias_f32(), BOFF))
    print("calibrated tables: weight_q", list(calibrated.weight_q), "bias_q", list(calibrated.bias_q), "act_q", list(calibrated.act_q))
    assert list(calibrated.weight_q) == wq and list(calibrated.bias_q) == bq and list(calibrated.act_q) == aq
    assert calibrated.act_q[0] == 14 and calibrated.clamped == 0 and calibrated.frames_seen == 1
    assert calibrated.act_absmax.tobytes() == want_act.tobytes()


def test_tables_with_headroom_and_the_concat_fixup(ctx, model, frames, oracle_stats):
    want_act, _ = oracle_stats
    ctx.calib_reset()
    ctx.calib_frames(frames[:1])
    w_max, b_max = layer_maxima(model.weights_f32(), WOFF), layer_maxima(model.bias_f32(), BOFF)
    for h in (1.0, 1.5, 4.0):
        got = ctx.calib_q_tables(h)
        assert [list(t) for t in got] == [list(t) for t in tables_by_rule(want_act, w_max, b_max, h)], h
    # layer 24's weights and biases at a quarter: its output Q rises above layer 26's, and the fix-up brings it back down
    w, b = model.weights_f32().copy(), model.bias_f32().copy()
    w[WOFF[ORD24]:WOFF[ORD24 + 1]] *= np.float32(0.25)
    b[BOFF[ORD24]:BOFF[ORD24 + 1]] *= np.float32(0.25)
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(w, b)
    c.calib_frames(frames[:1])
    st = c.calib_stats()
    wq, bq, aq = c.calib_q_tables(1.0)
    c.close()
    raw24, raw26 = q_rule(st["act_absmax"][ORD24 + 1]), q_rule(st["act_absmax"][ORD26 + 1])
    assert raw24 > raw26, (raw24, raw26)                      # the case is the one the fix-up is for
    assert aq[ORD24 + 1] == raw26 and aq[ORD26 + 1] == raw26
    assert list(aq) == tables_by_rule(st["act_absmax"], st["weight_absmax"], st["bias_absmax"])[2]
    assert wq[ORD24] == q_rule(w_max[ORD24] / 4)


# ------------------------------------------------------------------ 6. + 7. the calibrated model on the int16 pass

def test_calibrated_model_runs_bit_exactly_and_does_not_saturate(calibrated, calibrated_run, frames):
    region, q, layers = calibrated_run
    assert q == calibrated.act_q[NCONV]
    ri0, _, q0, dumps = oracle_i16(calibrated, frames[0], dump=True)
    ri1, _, q1 = oracle_i16(calibrated, frames[1])
    assert q0 == q and q1 == q
    assert np.array_equal(region[0].reshape(-1), ri0) and np.array_equal(region[1].reshape(-1), ri1)
    # frame 0 is the calibration frame: no int16 value of any layer sits at a saturation bound - in the tensors the pass materialised
    # (a conv fused with its pool leaves only the pooled tensor) and in the oracle's dump of every layer
    assert len(layers) >= 20
    for i, t in layers.items():
        assert saturated(t) == 0, f"layer {i}: {saturated(t)} values at a saturation bound"
    for i, t in dumps.items():
        assert saturated(t) == 0, f"oracle layer {i}: {saturated(t)} values at a saturation bound"
        if i in layers:
            assert np.array_equal(layers[i][:, :, :net.LAYERS[i].out_w], t[:, :, :net.LAYERS[i].out_w]), i


def test_calibrated_tables_are_closer_to_fp32_than_the_hand_picked_ones(ctx, model, calibrated_run, frames):
    region_cal, q_cal, _ = calibrated_run
    exact = ctx.run_batch_fp32_host(frames)
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)                                       # STD_Q: weight 14, bias 12, activations 9
    region_std, q_std = c.run_batch_host(frames)
    c.close()
    for f in range(2):
        e_cal = np.abs(region_cal[f].astype(np.float64) * 2.0 ** -q_cal - exact[f]).max()
        e_std = np.abs(region_std[f].astype(np.float64) * 2.0 ** -q_std - exact[f]).max()
        print(f"frame {f}: max |int16 region - fp32 region|  calibrated {e_cal:.6f}  STD_Q {e_std:.6f}")
        assert e_cal < e_std, (f, e_cal, e_std)


# ------------------------------------------------------------------ 8. full-mantissa weights

@pytest.fixture(scope="module")
def base_model():
    return synth.SynthModel(seed=1)


@pytest.mark.parametrize("spread", [0.5, 3.0])
def test_dense_model_gets_an_int16_form(base_model, frames, spread):
    dense = f16models.DenseModel(seed=1, spread=spread, base=base_model)
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(dense.weights_f32(), dense.bias_f32())
    cal = c.calibrate(frames=frames[:1], batch=1)
    exact = c.run_batch_fp32_host(frames[:1])[0]
    assert cal.clamped == 0 and cal.frames_seen == 1
    c.load_model(cal)
    region, q = c.run_batch_host(frames[:1])
    fused = c.pool_fused_layers()
    for l in net.LAYERS:
        if l.type in (net.CONV, net.MAXPOOL) and not (l.idx in fused and l.idx != 16):
            assert saturated(c.debug_layer_output(l.idx, 0)) == 0, l.idx
    c.close()
    ri, _, qo, dumps = oracle_i16(cal, frames[0], dump=True)
    assert qo == q and np.array_equal(region[0].reshape(-1), ri)
    for i, t in dumps.items():
        assert saturated(t) == 0, f"oracle layer {i}"
    err = np.abs(region[0].astype(np.float64) * 2.0 ** -q - exact)
    print(f"DenseModel(spread={spread}): act_q {list(cal.act_q)} weight_q {list(cal.weight_q)}; region error vs fp32 max {err.max():.6f} rms {np.sqrt((err ** 2).mean()):.6f}")


# ------------------------------------------------------------------ 9. refusals

def test_refusals_leave_the_context_usable(ctx, frames, oracle_stats):
    L = hipdrv.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: L.yolo2_hip_last_error().decode()
    bare = hipdrv.Yolo2Hip(0)                                 # no fp32 weights
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        bare.calib_frames(frames[:1])
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        bare.calib_images([np.zeros((8, 8, 3), np.uint8)], 1)
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        bare.calib_stats()
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        bare.calib_q_tables()
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        bare.quantize_weights([14] * NCONV, [12] * NCONV)
    bare.calib_reset()
    bare.close()
    ctx.calib_reset()
    with pytest.raises(hipdrv.Yolo2HipError, match="no calibration frame"):
        ctx.calib_q_tables()
    ctx.calib_frames(frames[:1])
    before = ctx.calib_stats()
    bad = frames[1:2].copy()
    bad[0, 2, 400, 17] = np.nan
    with pytest.raises(hipdrv.Yolo2HipError, match="non-finite"):
        ctx.calib_frames(bad)
    with pytest.raises(hipdrv.Yolo2HipError, match="non-finite"):
        ctx.calib_frames(np.concatenate([frames[:1], bad]))
    buf = hipdrv.DevBuf(frames[:1])
    for batch in (0, -1, 1025):
        assert L.yolo2_hip_calib_frames(ctx._h, buf.addr, batch, None) == hipdrv.YOLO2_ERROR and "out of range" in err()
    assert L.yolo2_hip_calib_frames(ctx._h, 0, 1, None) == hipdrv.YOLO2_ERROR and "null" in err()
    buf.free()
    n, ptrs, ws, hs, _, _keep = hipdrv._image_args([np.zeros((8, 8, 3), np.uint8)])
    assert L.yolo2_hip_calib_images_pix_host(ctx._h, ptrs, ws, hs, 7, n, 1) == hipdrv.YOLO2_ERROR and "unknown pixel format" in err()
    assert L.yolo2_hip_calib_images_pix_host(ctx._h, ptrs, ws, hs, 3, n, 0) == hipdrv.YOLO2_ERROR and "batch" in err()
    assert L.yolo2_hip_calib_images_pix_host(ctx._h, ptrs, ws, hs, 3, 0, 1) == hipdrv.YOLO2_ERROR and "count" in err()
    wq, bq = np.full(NCONV, 14, np.int32), np.full(NCONV, 12, np.int32)
    w, b = np.empty(hipdrv.N_WEIGHTS, np.int16), np.empty(hipdrv.N_BIAS, np.int16)
    q = lambda *a: L.yolo2_hip_quantize_weights_int16(ctx._h, *a)
    assert q(vp(wq), vp(bq), None, w.size, vp(b), b.size, None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert q(vp(wq), vp(bq), vp(w), w.size, None, b.size, None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert q(None, vp(bq), vp(w), w.size, vp(b), b.size, None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert q(vp(wq), vp(bq), vp(w), w.size - 1, vp(b), b.size, None) == hipdrv.YOLO2_ERROR and "short" in err()
    assert q(vp(wq), vp(bq), vp(w), w.size, vp(b), b.size - 1, None) == hipdrv.YOLO2_ERROR and "short" in err()
    wq[5] = 31
    assert q(vp(wq), vp(bq), vp(w), w.size, vp(b), b.size, None) == hipdrv.YOLO2_ERROR and "conv 5" in err()
    assert L.yolo2_hip_calib_q_tables(ctx._h, 1.0, None, vp(bq), vp(bq)) == hipdrv.YOLO2_ERROR and "null" in err()
    with pytest.raises(hipdrv.Yolo2HipError, match="headroom"):
        ctx.calib_q_tables(0.99)
    # nothing of that moved the statistics, and the context still calibrates
    after = ctx.calib_stats()
    assert after["frames_seen"] == 1 and after["act_absmax"].tobytes() == before["act_absmax"].tobytes() == oracle_stats[0].tobytes()
    assert [list(t) for t in ctx.calib_q_tables()] == [list(t) for t in tables_by_rule(after["act_absmax"], after["weight_absmax"], after["bias_absmax"])]


# ------------------------------------------------------------------ 10. the command-line tool

def test_calibrate_tool_writes_a_weight_set_the_detector_runs(tmp_path, base_model):
    images = np.load(os.path.join(orclib.ROOT, "tests", "golden", "images.npz"))
    names = ["jpg/base_444", "png/rgb", "jpg/big_420"]
    dense = f16models.DenseModel(seed=1, spread=0.5, base=base_model)
    wdir, idir, out = tmp_path / "weights", tmp_path / "imgs", tmp_path / "int16"
    wdir.mkdir()
    idir.mkdir()
    dense.weights_f32().tofile(str(wdir / "weights_reorg.bin"))
    dense.bias_f32().tofile(str(wdir / "bias.bin"))
    for k, name in enumerate(names):
        (idir / f"{k:02d}_{name.replace('/', '_')}.{name.split('/')[0]}").write_bytes(images[name + "/file"].tobytes())
    r = subprocess.run([os.path.join(PKG, "yolov2_calibrate"), "--weights", str(wdir), "--input-dir", str(idir), "--batch", "2", "--out", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "calibrated on 3 images" in r.stdout and "act_q" in r.stdout and "values clamped to +-32767: 0" in r.stdout
    assert sorted(os.listdir(out)) == sorted(hipdrv.CalibratedModel.FILES)
    cal = hipdrv.CalibratedModel.read_files(str(out))
    # the same images through hipdrv give the same set
    imgs = [images[name + "/rgb"] for name in names]
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(dense.weights_f32(), dense.bias_f32())
    lib_cal = c.calibrate(images=imgs, batch=2)
    assert lib_cal.frames_seen == 3
    for t in ("weight_q", "bias_q", "act_q"):
        assert np.array_equal(getattr(cal, t), getattr(lib_cal, t)), t
    assert np.array_equal(cal.weights_i16(), lib_cal.weights_i16()) and np.array_equal(cal.bias_i16(), lib_cal.bias_i16())
    # and batch 2 + a short last chunk saw what one chunk of 3 sees
    c.calib_reset()
    c.calib_images(imgs, 3)
    assert c.calib_stats()["act_absmax"].tobytes() == lib_cal.act_absmax.tobytes()
    c.load_model(cal)
    thresh, nms = 0.1, 0.45
    want = hipdrv.run_images_dets(c._h, imgs, 3, thresh, nms, cap=845, best_class=True)
    c.close()
    jsonl = tmp_path / "dets.jsonl"
    r = subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                        os.path.join(PKG, "config", "coco.names"), "--weights", str(out), "--precision", "int16", "--input-dir", str(idir),
                        "--batch", "3", "--thresh", str(thresh), "--nms", str(nms), "--jsonl", str(jsonl)],
                       capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, YOLO2_NO_DUMP="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = [json.loads(line) for line in jsonl.read_text().splitlines()]
    assert len(recs) == len(names)
    for k, rec in enumerate(recs):
        keep = [d for d in want["dets"][k] if d["prob"] > thresh]
        assert len(rec["detections"]) == len(keep), k
        for g, w in zip(rec["detections"], keep):
            assert g["class_id"] == int(w["cls"]) and g["prob"] == float("%.6f" % w["prob"])
            assert [g["bbox_norm"][c_] for c_ in "xywh"] == [float("%.6f" % w[c_]) for c_ in "xywh"]
