"""GPU tests of who owns device and pinned memory in libyolo2_hip.so: the live-bytes counters of the library's owners
(yolo2_hip_debug_live_bytes) return to where they were after a context's whole life and after every error return that needs no fault.
The device's free-memory figure is not used: other processes move it."""
import ctypes as C
import os

import numpy as np
import pytest

from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    m = synth.SynthModel(seed=1)   # the standard synthetic weight set of the parity tests
    return {"m": m, "w16": m.weights_i16(), "b16": m.bias_i16(), "w32": m.weights_f32(), "b32": m.bias_f32()}


@pytest.fixture(scope="module")
def frames2():
    return synth.frames(7, 2)      # frame 0 is the frame of tests/golden/fullnet.npz


def _fresh_ctx():
    ctx = hipdrv.Yolo2Hip(0)
    ctx.set_option("autotune", 0)  # static plans: nothing is timed
    return ctx


def _load_i16(ctx, model):
    ctx.load_weights(model["w16"], model["b16"], model["m"].weight_q, model["m"].bias_q, model["m"].act_q)


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, size=(48, 64, 3), dtype=np.uint8) for _ in range(3)]   # three 64 x 48 RGB images


def _cycle(model, frames2):
    """One context's whole life.  Returns the counters after every step, the region tensors / records of every run, and the
    readings around the reloads."""
    marks, outs = [], []
    mark = lambda: marks.append(hipdrv.live_bytes())
    tile = lambda n: np.ascontiguousarray(np.tile(frames2, (n // 2, 1, 1, 1)))
    ctx = _fresh_ctx()
    mark()
    _load_i16(ctx, model)
    mark()
    for b, lanes in ((2, 1), (16, 2), (2, 1)):
        outs.append(ctx.run_batch_host(tile(b))[0])
        assert ctx.num_lanes() == lanes
        mark()
    ctx.load_weights_fp32(model["w32"], model["b32"])
    mark()
    outs.append(ctx.run_batch_fp16_host(tile(2)))
    mark()
    outs.append(ctx.run_batch_fp16_host(tile(64)))
    assert ctx.num_lanes_fp16() == 2
    mark()
    outs.append(ctx.run_batch_f32tol_host(tile(2)))   # makes the split twin
    mark()
    outs.append(ctx.run_batch_fp32_host(frames2[:1]))
    mark()
    for precision in ("int16", "fp16"):               # fills PipeBufs, the post buffers and the pinned mirrors
        r = hipdrv.run_images_dets(ctx._h, _images(), 2, 0.1, 0.45, cap=64, precision=precision)
        outs.append(r["counts"])
        outs.extend(np.asarray(d).view(np.uint8) for d in r["dets"])
        mark()
    alive = hipdrv.live_bytes()
    # reload both weight sets on the live context, twice.  The int16 reload replaces buffers of the same sizes and no lane exists
    # (the last int16 batch was 2): nothing may change.  The first fp32 reload also destroys the fp16 lanes, the twin and the packed
    # fp32 weights: it may only shrink; the second replaces like with like.
    reload_marks = []
    for _ in range(2):
        before = hipdrv.live_bytes()
        _load_i16(ctx, model)
        mid = hipdrv.live_bytes()
        ctx.load_weights_fp32(model["w32"], model["b32"])
        reload_marks.append((before, mid, hipdrv.live_bytes()))
        outs.append(ctx.run_batch_host(frames2)[0])
        outs.append(ctx.run_batch_fp16_host(frames2))
        mark()
    ctx.close()
    mark()
    return marks, outs, alive, reload_marks


def test_lifecycle_balance(model, frames2):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))["i16/std/region_raw_i16"]
    start = hipdrv.live_bytes()
    cycles = [_cycle(model, frames2) for _ in range(2)]
    for k, (marks, outs, alive, reloads) in enumerate(cycles):
        print(f"cycle {k}: live (device, pinned) bytes per step {marks}; around the reloads {reloads}")
        assert marks[-1] == start, "the counters after close differ from those before the context was made"
        assert marks[0] == start and marks[1][0] > start[0], "the device counter does not move with the first weight load"
        assert alive[0] > start[0] and alive[1] > start[1], "the counters are not wired"
        (b1, m1, a1), (b2, m2, a2) = reloads
        assert m1 == b1 and m2 == b2, "reloading the int16 weights changed the live bytes"
        assert a1[0] <= m1[0] and a1[1] == m1[1], "the first fp32 reload grew the live bytes"
        assert a2 == m2, "the second fp32 reload changed the live bytes"
        assert marks[-2] == marks[-3], "the same point after the second reload holds other bytes than after the first"
        assert np.array_equal(outs[0][0].reshape(-1), golden), "int16 region tensor differs from the reference fixture"
    assert cycles[1][0] == cycles[0][0], "the second cycle's readings differ from the first's"
    assert cycles[1][3] == cycles[0][3]
    assert len(cycles[0][1]) == len(cycles[1][1])
    for a, b in zip(cycles[0][1], cycles[1][1]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), "outputs differ between cycles"


def test_error_returns_leave_the_counters_alone(model, frames2):
    """Error returns behind an allocation that need no fault: the code and the message are set, the counters do not move, and the
    context still computes the reference's region tensor afterwards."""
    L = hipdrv.lib()
    golden = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))["i16/std/region_raw_i16"]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    region = np.empty((2, 425, 13, 13), dtype=np.float32)

    def refused(call, what):
        before = hipdrv.live_bytes()
        rc = call()
        msg = L.yolo2_hip_last_error().decode()
        after = hipdrv.live_bytes()
        print(f"{what}: status {rc}, '{msg}', live bytes {before} -> {after}")
        assert rc == hipdrv.YOLO2_ERROR and msg, what
        assert after == before, f"{what}: the live bytes moved"
        return msg

    ctx = _fresh_ctx()
    _load_i16(ctx, model)
    ref16 = ctx.run_batch_host(frames2)[0]
    assert np.array_equal(ref16[0].reshape(-1), golden)
    # no fp32 weights: the staging buffers are allocated, then the pass refuses
    for name in ("yolo2_hip_run_batch_fp16_host", "yolo2_hip_run_batch_f32tol_host"):
        msg = refused(lambda: getattr(L, name)(ctx._h, vp(frames2), 2, vp(region)), name + " without fp32 weights")
        assert "fp32 weights not loaded" in msg
    # the blobs are uploaded, then load_common refuses the empty activation Q table
    m = model["m"]
    wq, bq, aq = (np.ascontiguousarray(a, dtype=np.int32) for a in (m.weight_q, m.bias_q, m.act_q))
    msg = refused(lambda: L.yolo2_hip_load_weights_int16(ctx._h, vp(model["w16"]), model["w16"].size, vp(model["b16"]), model["b16"].size,
                                                         vp(wq), wq.size, vp(bq), bq.size, vp(aq), 0), "yolo2_hip_load_weights_int16 with n_act_q = 0")
    assert "iofm_Q" in msg
    assert np.array_equal(ctx.run_batch_host(frames2)[0], ref16), "the context computes something else after the refused load"
    # batch 4097: the range check runs after the staging buffers (8.5 GB of frames) are allocated and filled
    ctx.load_weights_fp32(model["w32"], model["b32"])
    ref_h = ctx.run_batch_fp16_host(frames2)
    big = np.zeros((4097, 3, 416, 416), dtype=np.float32)
    big_region = np.empty((4097, 425, 13, 13), dtype=np.float32)
    msg = refused(lambda: L.yolo2_hip_run_batch_fp16_host(ctx._h, vp(big), 4097, vp(big_region)), "yolo2_hip_run_batch_fp16_host at batch 4097")
    assert "out of range" in msg
    del big, big_region
    assert np.array_equal(ctx.run_batch_fp16_host(frames2), ref_h), "the fp16 pass computes something else after the refused batch"
    assert np.array_equal(ctx.run_batch_host(frames2)[0], ref16)
    ctx.close()
