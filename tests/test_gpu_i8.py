"""The int8 pass on the GPU (run with -m gpu): every check is equality against tests/i8ref.py, the arithmetic of
include/yolo2_hip.h "int8 pass" in float64.  int32 accumulation is exact, so no tiling or k order may change a bit."""
import os
import subprocess

import numpy as np
import pytest

import i8ref
import orclib
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def driver():
    L = hipdrv.lib()
    assert L.yolo2_hip_device_count() >= 1, "no GPU visible: these tests must run on the GPU box"
    hipdrv.check(L.yolo2_accel_init(), "yolo2_accel_init")
    yield L
    L.yolo2_accel_cleanup()


# ------------------------------------------------------------------ single layers through the driver tier

def _run_case(x, w, b, qw, q_in, q_out, leaky, fout=False):
    want = i8ref.conv(x, w, b, qw, q_in, q_out, leaky, out_float=fout)
    got, g0, g1 = hipdrv.conv_layer_i8(x, w, b, qw, q_in, q_out, leaky, out_float=fout)
    assert g0.size == 128 and (g0 == 0xA5).all(), "the guard in front of the output was written"
    assert g1.size >= 128 and (g1 == 0xA5).all(), "the guard behind the output was written"
    assert got.shape == want.shape and got.dtype == want.dtype
    if fout:
        same = got.view(np.uint32) == want.view(np.uint32)
    else:
        same = got == want
    assert same.all(), f"{int((~same).sum())} of {same.size} differ, first at {tuple(np.argwhere(~same)[0])}"
    return want


def test_case1_three_channels_padded_to_the_k_granule():
    rng = np.random.default_rng(11)
    x = rng.integers(-128, 128, (2, 3, 8, 8)).astype(np.int8)
    w = rng.integers(-127, 128, (32, 3, 3, 3)).astype(np.int8)
    y = _run_case(x, w, rng.integers(-20000, 20000, 32).astype(np.int32), rng.integers(6, 9, 32).astype(np.int32), 6, 2, True)
    assert -128 < y.min() and y.max() < 127 and y.std() > 10       # the shifts leave the values inside int8: no clamp hides a bit


def test_case2_odd_size_tile_tails_and_frame_strides():
    rng = np.random.default_rng(12)
    x = rng.integers(-128, 128, (3, 32, 13, 13)).astype(np.int8)
    w = rng.integers(-127, 128, (64, 32, 3, 3)).astype(np.int8)
    y = _run_case(x, w, rng.integers(-50000, 50000, 64).astype(np.int32), rng.integers(7, 10, 64).astype(np.int32), 6, 1, True)
    assert -128 < y.min() and y.max() < 127 and y.std() > 5 and not np.array_equal(y[0], y[1])


def test_case3_channel_tail_and_float_output_above_2_pow_24():
    rng = np.random.default_rng(13)
    x = rng.integers(-128, 128, (2, 64, 13, 13)).astype(np.int8)
    w = rng.integers(-127, 128, (425, 64, 1, 1)).astype(np.int8)
    b = rng.integers(-2 ** 29, 2 ** 29, 425).astype(np.int32) | 1      # odd accumulators far above 2^24: int -> float must round
    qw = rng.integers(-8, 25, 425).astype(np.int32)
    acc = i8ref._acc(x, w, b)
    assert (np.abs(acc) > 2 ** 24).mean() > 0.9 and (acc.astype(np.float32).astype(np.float64) != acc).mean() > 0.5
    _run_case(x, w, b, qw, 6, 0, False, fout=True)


def test_case4_largest_reachable_accumulator():
    rng = np.random.default_rng(14)
    x = np.where(rng.random((2, 1280, 13, 13)) < 0.5, -128, 127).astype(np.int8)
    x[0] = -128
    w = np.where(rng.random((32, 1280, 3, 3)) < 0.5, -127, 127).astype(np.int8)
    w[0], w[1] = -127, 127
    b = rng.integers(-1000, 1000, 32).astype(np.int32)
    qw = rng.integers(19, 22, 32).astype(np.int32)
    acc = i8ref._acc(x, w, b)
    assert acc.max() == 1280 * 9 * 127 * 128 + b[0] and acc.min() == -1280 * 9 * 127 * 128 + b[1]
    y = _run_case(x, w, b, qw, 6, 5, True)
    assert y.max() > 40 and y.min() < -3


def test_case5_small_accumulators_every_shift_kind_and_saturation():
    rng = np.random.default_rng(15)
    x = rng.integers(-2, 3, (1, 64, 26, 26)).astype(np.int8)
    w = np.zeros((64, 64 * 9), dtype=np.int8)
    for m in range(64):                                           # three taps of +-1 per output channel: |sum| <= 6
        w[m, rng.choice(64 * 9, 3, replace=False)] = rng.choice([-1, 1], 3)
    w = w.reshape(64, 64, 3, 3)
    b = rng.integers(-3, 4, 64).astype(np.int32)
    b[60:] = -5000                                                # leaky leaves -500: saturates at -128 where s <= 1
    qw = np.array([2, 0, -3, 1, -7, 3, 0, -1] * 8, dtype=np.int32)     # s = qw: s > 0, s = 0, s = -3, ... inside every 32-channel block
    acc = i8ref._acc(x, w, b)
    assert acc[:, :60].min() >= -9 and acc[:, :60].max() <= 9 and (acc[:, :60] < 0).any()
    y = _run_case(x, w, b, qw, 0, 0, True)
    assert (y == 127).any() and (y == -128).any()
    assert (y[:, :60] >= 0).all()                                 # -9..-1 divided by 10 truncates to 0; a floor would give -1


@pytest.mark.parametrize("K,tap", [(1, (0, 0)), (3, (1, 1)), (3, (0, 2)), (3, (2, 1))])
def test_case6_identity_weights_asymmetric_input(K, tap):
    """out[m] = x[m] (or x[m] one pixel over, for an off-centre tap): a transposed or permuted fragment map, a swapped row/column of
    the result or a mirrored tap cannot survive an input that differs in every channel, row and column."""
    B, C, H, W = 2, 64, 13, 9
    b_, c_, y_, x_ = np.meshgrid(np.arange(B), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    x = ((c_ * 37 + y_ * 11 + x_ * 5 + b_ * 101) % 251 - 125).astype(np.int8)
    w = np.zeros((64, 64, K, K), dtype=np.int8)
    w[np.arange(64), np.arange(64), tap[0], tap[1]] = 1
    y = _run_case(x, w, np.zeros(64, np.int32), np.zeros(64, np.int32), 0, 0, False)
    dy, dx = tap[0] - K // 2, tap[1] - K // 2
    want = np.zeros_like(x)
    ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
    yd, xd = slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx))
    want[:, :, ys, xs] = x[:, :, yd, xd]
    assert np.array_equal(y, want)                                # (the reference itself is pinned here, independently of torch)


def test_driver_entry_refuses_before_launching():
    x = np.zeros((1, 4, 4, 4), np.int8)
    w = np.full((2, 4, 3, 3), 127, np.int8)
    ok = dict(bias32=np.zeros(2, np.int32), weight_q=np.zeros(2, np.int32), q_in=0, q_out=0, leaky=False)
    hipdrv.conv_layer_i8(x, w, **ok)
    with pytest.raises(hipdrv.Yolo2HipError, match="shift"):
        hipdrv.conv_layer_i8(x, w, **dict(ok, q_in=24, weight_q=np.full(2, 24, np.int32), q_out=-8))
    with pytest.raises(hipdrv.Yolo2HipError, match="channel 1"):
        hipdrv.conv_layer_i8(x, w, **dict(ok, bias32=np.array([0, 2 ** 30], np.int32)))
    with pytest.raises(hipdrv.Yolo2HipError, match="not 1 or 3"):
        hipdrv.conv_layer_i8(np.zeros((1, 4, 5, 5), np.int8), np.zeros((2, 4, 5, 5), np.int8), **ok)


# ------------------------------------------------------------------ the whole network

class Net:
    pass


@pytest.fixture(scope="module")
def netw():
    """SynthModel(seed=1) calibrated on the GPU from synth.frames(40, 4); the reference quantised from the same maxima; the region
    tensor of synth.frames(41, 2) from both.  Computed once, shared, left unchanged."""
    n = Net()
    n.model = synth.SynthModel(seed=1)
    n.ctx = hipdrv.Yolo2Hip(0)
    n.ctx.load_weights_fp32(n.model.weights_f32(), n.model.bias_f32())
    n.cal = n.ctx.calibrate_int8(frames=synth.frames(40, 4), batch=4)
    w, b = i8ref.model_f32(n.model)
    n.ref = i8ref.ModelI8(w, b, i8ref.act_q_from_stats(n.cal.act_absmax, 1.0))
    n.ctx.load_model(n.cal)
    n.frames = synth.frames(41, 5)
    n.region = n.ctx.run_batch_int8_host(n.frames[:2])
    n.layers = {i: n.ctx.debug_i8_tensor(i, 1) for i in range(-1, 30) if net.LAYERS[max(i, 0)].type != net.ROUTE or i == 28}
    n.want, n.want_layers = i8ref.forward(n.frames[:2], n.ref, keep=True)
    yield n
    n.ctx.close()


def test_quantiser_equals_the_reference_from_the_same_maxima(netw):
    w8, b32, qw = netw.ref.flat()
    assert netw.cal.frames_seen == 4
    assert np.array_equal(netw.cal.act_q, netw.ref.act_q) and netw.cal.act_q[0] == 6 and netw.cal.act_q[20] == netw.cal.act_q[21]
    assert np.array_equal(netw.cal.weight_q, qw)
    assert np.array_equal(netw.cal.bias32, b32)
    assert np.array_equal(netw.cal.w8, w8)
    assert np.abs(netw.cal.w8.astype(np.int16)).max() == 127


def test_whole_network_region_is_float_equal(netw):
    if not np.array_equal(netw.region.view(np.uint32), netw.want.view(np.uint32)):
        for i in sorted(netw.layers):                             # the parity hook names the first layer that went wrong
            got, q = netw.layers[i]
            want = netw.want_layers[i][1]
            if got.shape != want.shape or not np.array_equal(got, want):
                pytest.fail(f"first differing layer: {i} ({int((got != want).sum()) if got.shape == want.shape else got.shape} of {want.size})")
        pytest.fail("every int8 tensor equals the reference; layer 30's float store differs")
    assert np.isfinite(netw.region).all() and netw.region.std() > 0.1


def test_parity_hook_reads_every_tensor_of_the_last_run(netw):
    for i, (got, q) in netw.layers.items():
        assert np.array_equal(got, netw.want_layers[i][1]), f"layer {i}"
    assert netw.layers[-1][1] == netw.cal.act_q[0] and netw.layers[0][1] == netw.cal.act_q[1] and netw.layers[1][1] == netw.cal.act_q[1]
    assert netw.layers[28][0].shape == (1280, 13, 13) and netw.layers[27][0].shape == (256, 13, 13)
    with pytest.raises(hipdrv.Yolo2HipError):
        netw.ctx.debug_i8_tensor(30, 0)
    with pytest.raises(hipdrv.Yolo2HipError):
        netw.ctx.debug_i8_tensor(0, 2)


def test_batch5_equals_batch1_frame_by_frame(netw):
    r5 = netw.ctx.run_batch_int8_host(netw.frames)
    assert np.array_equal(r5[:2].view(np.uint32), netw.region.view(np.uint32))
    for f in range(5):
        r1 = netw.ctx.run_batch_int8_host(netw.frames[f:f + 1])
        assert np.array_equal(r1[0].view(np.uint32), r5[f].view(np.uint32)), f"frame {f}"
    netw.ctx.run_batch_int8_host(netw.frames[:2])                 # (leaves the two-frame run behind for the hook's users)


def test_loader_refusals_leave_the_loaded_set_alone(netw):
    c, ld = netw.cal, netw.ctx.load_weights_int8
    aq = c.act_q.copy()
    aq[20] += 1
    with pytest.raises(hipdrv.Yolo2HipError, match=r"act_q\[20\]"):
        ld(c.w8, c.bias32, c.weight_q, aq)
    aq = c.act_q.copy()
    aq[1] = -8
    wq = c.weight_q.copy()
    wq[3] = 24                                                    # s = 6 + 24 + 8 = 38
    with pytest.raises(hipdrv.Yolo2HipError, match=r"conv 0 \(layer 0\), channel 3: shift"):
        ld(c.w8, c.bias32, wq, aq)
    wq = c.weight_q.copy()
    wq[5] = 25
    with pytest.raises(hipdrv.Yolo2HipError, match="weight Q 25"):
        ld(c.w8, c.bias32, wq, c.act_q)
    b = c.bias32.copy()
    b[32 + 7] = -2 ** 30
    with pytest.raises(hipdrv.Yolo2HipError, match=r"conv 1 \(layer 2\), channel 7: .*2\^31"):
        ld(c.w8, b, c.weight_q, c.act_q)
    with pytest.raises(hipdrv.Yolo2HipError, match="weights"):
        ld(c.w8[:-1], c.bias32, c.weight_q, c.act_q)
    with pytest.raises(hipdrv.Yolo2HipError, match="channels"):
        ld(c.w8, c.bias32[:-1], c.weight_q[:-1], c.act_q)
    again = netw.ctx.run_batch_int8_host(netw.frames[:2])
    assert np.array_equal(again.view(np.uint32), netw.region.view(np.uint32))
    fresh = hipdrv.Yolo2Hip(0)
    try:
        with pytest.raises(hipdrv.Yolo2HipError, match="int8 weights not loaded"):
            fresh.run_batch_int8_host(netw.frames[:1])
    finally:
        fresh.close()


@pytest.mark.parametrize("tail", ["core", "app"])
def test_float_tail_on_the_int8_region(netw, tail):
    """hipdrv.postprocess on the region tensor the int8 pass left in HBM returns the records of the float tail on i8ref's tensor."""
    iw, ih = [640, 500], [480, 375]
    out = hipdrv.DevBuf(nbytes=netw.want.nbytes)
    fr = hipdrv.DevBuf(netw.frames[:2])
    ref = hipdrv.DevBuf(netw.want)
    try:
        netw.ctx.run_batch_int8_ptr(fr.addr, 2, out.addr)
        got = hipdrv.postprocess(netw.ctx, out.addr, 2, iw, ih, 0.005, 0.45, cap=845, tail=tail)
        want = hipdrv.postprocess(netw.ctx, ref.addr, 2, iw, ih, 0.005, 0.45, cap=845, tail=tail)
    finally:
        for d in (out, fr, ref):
            d.free()
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"].min() > 0
    for f in range(2):
        assert got["dets"][f].tobytes() == want["dets"][f].tobytes()


def test_other_passes_on_the_same_context_are_unchanged():
    model = synth.SynthModel(seed=1)
    frames = synth.frames(41, 2)
    ctx = hipdrv.Yolo2Hip(0)
    try:
        ctx.load_model(model)
        ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
        r16, q16 = ctx.run_batch_host(frames)
        f16 = ctx.run_batch_fp16_host(frames)
        ctx.load_model(ctx.calibrate_int8(frames=synth.frames(40, 2), batch=2))
        r8 = ctx.run_batch_int8_host(frames)
        r16b, q16b = ctx.run_batch_host(frames)
        f16b = ctx.run_batch_fp16_host(frames)
        assert q16 == q16b and np.array_equal(r16, r16b)
        assert np.array_equal(f16.view(np.uint32), f16b.view(np.uint32))
        assert np.array_equal(ctx.run_batch_int8_host(frames).view(np.uint32), r8.view(np.uint32))
        assert np.sqrt(np.mean((r8 - f16) ** 2)) < 0.5             # the three passes run the same network
    finally:
        ctx.close()


# ------------------------------------------------------------------ the command line

def test_calibrate_and_detect_tools_run_the_int8_set(tmp_path):
    """yolov2_calibrate --format int8 writes the four files Yolo2Hip.calibrate_int8 makes from the same images, and
    yolov2_detect --precision int8 on them dumps the region tensor the library returns for the same letterboxed frame."""
    pkg = hipdrv.PKG_DIR
    images = np.load(os.path.join(orclib.ROOT, "tests", "golden", "images.npz"))
    names = ["jpg/base_444", "png/rgb"]
    model = synth.SynthModel(seed=1)
    wdir, idir, out = tmp_path / "weights", tmp_path / "imgs", tmp_path / "int8"
    wdir.mkdir()
    idir.mkdir()
    model.weights_f32().tofile(str(wdir / "weights_reorg.bin"))
    model.bias_f32().tofile(str(wdir / "bias.bin"))
    for k, name in enumerate(names):
        (idir / f"{k:02d}_{name.replace('/', '_')}.{name.split('/')[0]}").write_bytes(images[name + "/file"].tobytes())
    r = subprocess.run([os.path.join(pkg, "yolov2_calibrate"), "--format", "int8", "--weights", str(wdir), "--input-dir", str(idir), "--batch", "2",
                        "--out", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "calibrated on 2 images" in r.stdout and "int8" in r.stdout
    assert sorted(os.listdir(out)) == sorted(hipdrv.CalibratedModelI8.FILES)
    cal = hipdrv.CalibratedModelI8.read_files(str(out))
    ctx = hipdrv.Yolo2Hip(0)
    try:
        ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
        lib_cal = ctx.calibrate_int8(images=[images[n + "/rgb"] for n in names], batch=2)
        for t in ("act_q", "weight_q", "bias32", "w8"):
            assert np.array_equal(getattr(cal, t), getattr(lib_cal, t)), t
        img = np.random.default_rng(5).integers(0, 256, (300, 500, 3), dtype=np.uint8)
        ppm = tmp_path / "img.ppm"
        ppm.write_bytes(b"P6\n500 300\n255\n" + img.tobytes())
        env = dict(os.environ, YOLO2_DUMP_REGION_RAW=str(tmp_path / "raw.txt"), YOLO2_DUMP_REGION=str(tmp_path / "proc.txt"))
        for batch in ("1", "3"):
            r = subprocess.run([os.path.join(pkg, "yolov2_detect"), "--cfg", os.path.join(pkg, "config", "yolov2.cfg"), "--names",
                                os.path.join(pkg, "config", "coco.names"), "--weights", str(out), "--input", str(ppm), "--output",
                                str(tmp_path / "pred"), "--thresh", "0.01", "--batch", batch, "--precision", "int8"],
                               capture_output=True, text=True, env=env, cwd=str(tmp_path))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "precision: int8" in r.stdout and "detection(s) above 0.01" in r.stdout
            chw = img.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            boxed = np.zeros((3, 416, 416), dtype=np.float32)
            orclib.host().y2h_letterbox(np.ascontiguousarray(chw), 500, 300, 3, 416, 416, boxed)
            ctx.load_model(cal)
            region = ctx.run_batch_int8_host(boxed[None])
            raw = np.loadtxt(tmp_path / "raw.txt").astype(np.float32)
            assert np.array_equal(raw.view(np.uint32), region[0].reshape(-1).view(np.uint32))
    finally:
        ctx.close()
