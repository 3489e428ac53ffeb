"""The int8 pass without a GPU: the reference restatement against plain integer loops, the Q rule through the C ABI, the weight
set's files, the CLI's streaming refusal, and the accuracy of the DEFINITION (tests/i8ref.py against the float pass in float64)."""
import os
import subprocess

import numpy as np
import pytest

import i8ref
from yolo2_amd import hipdrv, net, synth

DETECT = os.path.join(hipdrv.PKG_DIR, "yolov2_detect")


@pytest.mark.parametrize("C,N,K,H,W,B,leaky,q_in,q_out,fout", [
    (3, 4, 3, 5, 4, 2, True, 6, 4, False),      # rounding shifts s > 0, borders on every side
    (5, 3, 1, 3, 3, 1, False, 0, 9, False),     # s <= 0: left shifts and saturation
    (4, 6, 3, 4, 4, 1, True, 5, 0, True),       # float output, leaky on the accumulator
])
def test_i8ref_conv_equals_a_plain_integer_loop(C, N, K, H, W, B, leaky, q_in, q_out, fout):
    rng = np.random.default_rng(C * 100 + N)
    x = rng.integers(-128, 128, (B, C, H, W)).astype(np.int8)
    w = rng.integers(-127, 128, (N, C, K, K)).astype(np.int8)
    b = rng.integers(-5000, 5000, N).astype(np.int32)
    qw = rng.integers(4, 9, N).astype(np.int32) if q_out != 9 else rng.integers(2, 7, N).astype(np.int32)
    got = i8ref.conv(x, w, b, qw, q_in, q_out, leaky, out_float=fout)
    want = i8ref.conv_loop(x, w, b, qw, q_in, q_out, leaky, out_float=fout)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    if not fout:
        assert got.min() < 0 < got.max()


def test_q8_rule_on_explicit_maxima():
    hipdrv.build()
    base = np.full(24, 1.0, dtype=np.float32)
    assert list(hipdrv.q8_from_stats(base)) == [6] * 24                      # 1.0 -> 6: 64 < 127.5 <= 128
    a = base.copy()
    a[0], a[3] = 0.0, 0.0
    q = hipdrv.q8_from_stats(a)
    assert q[0] == 24 and q[3] == 24                                          # an all-zero tensor takes the largest Q
    edge = np.float32(127.5 / 64)                                             # exactly on the boundary at q = 6: not below it
    a = base.copy()
    a[5], a[6] = edge, np.nextafter(edge, np.float32(0))
    q = hipdrv.q8_from_stats(a)
    assert q[5] == 5 and q[6] == 6
    q = hipdrv.q8_from_stats(base, headroom=2.0)                              # headroom on the conv outputs only
    assert q[0] == 6 and list(q[1:]) == [5] * 23
    a = base.copy()
    a[20], a[21] = 3.0, 0.3                                                   # layer 24 / layer 26: both take the smaller Q
    q = hipdrv.q8_from_stats(a)
    assert q[20] == q[21] == 5
    a[20], a[21] = 0.3, 3.0
    q = hipdrv.q8_from_stats(a)
    assert q[20] == q[21] == 5
    a = base.copy()
    a[2] = 127.5 * 2.0 ** 8                                                   # the smallest Q, -8, does not hold it
    with pytest.raises(hipdrv.Yolo2HipError, match="conv 1"):
        hipdrv.q8_from_stats(a)
    a[2] = np.nextafter(np.float32(127.5 * 2.0 ** 8), np.float32(0))
    assert hipdrv.q8_from_stats(a)[2] == -8
    a[2] = np.nan
    with pytest.raises(hipdrv.Yolo2HipError):
        hipdrv.q8_from_stats(a)
    with pytest.raises(hipdrv.Yolo2HipError, match="headroom"):
        hipdrv.q8_from_stats(base, headroom=0.5)
    rng = np.random.default_rng(3)
    for _ in range(20):                                                       # ... and the restatement agrees on arbitrary maxima
        a = (rng.random(24) * 10.0 ** rng.integers(-3, 3, 24)).astype(np.float32)
        h = float(rng.choice([1.0, 1.25, 2.0]))
        assert np.array_equal(hipdrv.q8_from_stats(a, h), i8ref.act_q_from_stats(a, h))


def test_calibrated_model_i8_file_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    m = hipdrv.CalibratedModelI8(rng.integers(-127, 128, net.N_WEIGHTS, dtype=np.int8), rng.integers(-2 ** 20, 2 ** 20, net.N_BIAS, dtype=np.int32),
                                 rng.integers(-8, 25, net.N_BIAS, dtype=np.int32), rng.integers(-8, 25, 24, dtype=np.int32))
    paths = m.write_files(str(tmp_path / "w8"))
    assert sorted(os.path.basename(p) for p in paths.values()) == sorted(hipdrv.CalibratedModelI8.FILES)
    assert sorted(os.listdir(tmp_path / "w8")) == sorted(("weights_int8.bin", "bias_int32.bin", "weight_int8_Q.bin", "iofm_int8_Q.bin"))
    assert os.path.getsize(paths["weights_int8.bin"]) == net.N_WEIGHTS and os.path.getsize(paths["bias_int32.bin"]) == 4 * net.N_BIAS
    r = hipdrv.CalibratedModelI8.read_files(str(tmp_path / "w8"))
    for name in ("w8", "bias32", "weight_q", "act_q"):
        assert np.array_equal(getattr(r, name), getattr(m, name)) and getattr(r, name).dtype == getattr(m, name).dtype
    with pytest.raises(ValueError):
        hipdrv.CalibratedModelI8(m.w8[:-1], m.bias32, m.weight_q, m.act_q)


def test_cli_refuses_int8_when_streaming(tmp_path):
    hipdrv.build()
    for src in (["--input-dir", str(tmp_path)], ["--input-list", str(tmp_path / "list.txt")]):
        r = subprocess.run([DETECT, "--precision", "int8", "--weights", str(tmp_path)] + src, capture_output=True, text=True)
        assert r.returncode == 1 and "int8" in r.stderr and "streaming" in r.stderr, r.stderr
    r = subprocess.run([DETECT, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "int8" in r.stdout
    r = subprocess.run([os.path.join(hipdrv.PKG_DIR, "yolov2_calibrate"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--format" in r.stdout and "weights_int8.bin" in r.stdout


@pytest.mark.slow
def test_int8_definition_is_int8_grade_against_the_float_pass():
    """SynthModel(seed=1), calibrated on synth.frames(40, 4), evaluated on synth.frames(41, 2): i8ref against the float pass in
    float64 on the same weights.  Measured when the arithmetic was defined: rms 0.092 (region std 0.94), mean box IoU 0.836; the
    bounds leave 1.5x on the error and 10 % on the IoU for restatement detail (fp32 versus fp64 maxima)."""
    model = synth.SynthModel(seed=1)
    w, b = i8ref.model_f32(model)
    _, absmax = i8ref.float_forward(synth.frames(40, 4), w, b)
    act_q = i8ref.act_q_from_stats(absmax, 1.0)
    m = i8ref.ModelI8(w, b, act_q)
    ev = synth.frames(41, 2)
    want, _ = i8ref.float_forward(ev, w, b)
    got = i8ref.forward(ev, m).astype(np.float64)
    rms = float(np.sqrt(np.mean((got - want) ** 2)))
    iou = i8ref.mean_iou(got, want)
    print(f"int8 definition vs float pass: act_q {act_q.min()}..{act_q.max()}, region rms error {rms:.4f} (std {want.std():.3f}, "
          f"max {np.abs(got - want).max():.3f}), mean box IoU {iou:.4f}")
    assert rms <= 0.14
    assert iou >= 0.75
