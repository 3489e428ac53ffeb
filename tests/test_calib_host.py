"""Calibration tier, the parts that need no GPU: the entries exist (header, library, hipdrv.EXPORTS), the Q rule on explicit
maxima (yolo2_hip_calib_q_from_stats: host arithmetic), argument refusals that are made before any device call, the command-line
tool's usage text, and the five files of a CalibratedModel read back."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv, net, synth

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CALIBRATE = os.path.join(PKG, "yolov2_calibrate")
ENTRIES = ["yolo2_hip_absmax_f32", "yolo2_hip_calib_reset", "yolo2_hip_calib_frames", "yolo2_hip_calib_images_pix_host",
           "yolo2_hip_calib_stats", "yolo2_hip_calib_q_tables", "yolo2_hip_calib_q_from_stats", "yolo2_hip_quantize_weights_int16"]
NCONV = len(net.CONVS)
ORD24 = next(l.ord for l in net.CONVS if l.idx == 24)   # conv ordinals of layers 24 and 26: the two halves of the concat tensor
ORD26 = next(l.ord for l in net.CONVS if l.idx == 26)


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "yolo2_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(hipdrv.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/yolo2_hip.h"
        assert hasattr(L, name), f"libyolo2_hip.so does not export {name}"
        assert name in hipdrv.EXPORTS, f"hipdrv.EXPORTS lacks {name}"
    for meth in ("calibrate", "calib_frames", "calib_images", "calib_stats", "calib_q_tables", "calib_reset", "quantize_weights"):
        assert callable(getattr(hipdrv.Yolo2Hip, meth))


def _tables(act=None, w=None, b=None, headroom=1.0):
    a = np.ones(NCONV + 1, np.float32) if act is None else np.asarray(act, np.float32)
    w = np.ones(NCONV, np.float32) if w is None else np.asarray(w, np.float32)
    b = np.ones(NCONV, np.float32) if b is None else np.asarray(b, np.float32)
    return hipdrv.q_tables_from_stats(a, w, b, headroom)


# the issue's cases: m -> q(m, 1).  3.9999 * 2^13 = 32767.18 still rounds to 32767, 4.0 * 2^13 = 32768 does not
Q_CASES = [(0.0, 15), (32767 * 2.0 ** -15, 15), (1.0, 14), (3.9999, 13), (4.0, 12), (32767.0, 0)]


@pytest.mark.parametrize("m,q", Q_CASES)
def test_q_rule_cases(m, q):
    """every table applies the same q(m, 1): the weight, the bias, the input and (headroom 1) a conv output"""
    for slot in range(4):
        act, w, b = np.ones(NCONV + 1, np.float32), np.ones(NCONV, np.float32), np.ones(NCONV, np.float32)
        [w, b, act, act][slot][[3, 3, 0, 5][slot]] = m
        wq, bq, aq = _tables(act, w, b)
        got = [wq[3], bq[3], aq[0], aq[5]][slot]
        assert got == q, (slot, m, got)
        assert (wq == 14).sum() + (bq == 14).sum() + (aq == 14).sum() == 3 * NCONV + 1 - (q != 14)


@pytest.mark.parametrize("slot", range(4))
def test_q_rule_refuses_a_maximum_no_q_holds(slot):
    act, w, b = np.ones(NCONV + 1, np.float32), np.ones(NCONV, np.float32), np.ones(NCONV, np.float32)
    [w, b, act, act][slot][[3, 3, 0, 5][slot]] = 32768.0
    with pytest.raises(hipdrv.Yolo2HipError, match=["weights of conv 3", "biases of conv 3", "network input", "output of conv 4"][slot]):
        _tables(act, w, b)
    for bad in (np.inf, np.nan):
        act[5] = bad
        with pytest.raises(hipdrv.Yolo2HipError):
            _tables(act, w, b)


def test_q_rule_headroom_applies_to_conv_outputs_only():
    act = np.full(NCONV + 1, 3.0, np.float32)      # 3 * 2^13 = 24576 fits; with headroom 2: 6 * 2^13 does not, 6 * 2^12 does
    act[0] = 1.0
    w, b = np.full(NCONV, 3.0, np.float32), np.full(NCONV, 3.0, np.float32)
    wq, bq, aq = _tables(act, w, b, headroom=1.0)
    assert (wq == 13).all() and (bq == 13).all() and aq[0] == 14 and (aq[1:] == 13).all()
    wq, bq, aq = _tables(act, w, b, headroom=2.0)
    assert (wq == 13).all() and (bq == 13).all() and aq[0] == 14 and (aq[1:] == 12).all()
    act[7] = 16383.0                               # headroom 2: 32766 fits at q = 0; headroom 2.001 leaves no q
    assert _tables(act, w, b, headroom=2.0)[2][7] == 0
    with pytest.raises(hipdrv.Yolo2HipError, match="output of conv 6"):
        _tables(act, w, b, headroom=2.001)
    for bad in (0.5, 0.0, -1.0, np.nan, np.inf):
        with pytest.raises(hipdrv.Yolo2HipError, match="headroom"):
            _tables(act, w, b, headroom=bad)


def test_q_rule_concat_fixup():
    """layer 24's output Q above layer 26's is lowered to it (the reorg half is only ever shifted down); below it, it stays"""
    act = np.full(NCONV + 1, 3.0, np.float32)
    act[ORD24 + 1], act[ORD26 + 1] = 0.7, 3.0      # raw rule: 15 and 13
    aq = _tables(act)[2]
    assert aq[ORD26 + 1] == 13 and aq[ORD24 + 1] == 13
    assert (np.delete(aq, [0, ORD24 + 1]) == 13).all()
    act[ORD24 + 1], act[ORD26 + 1] = 3.0, 0.7      # 13 and 15: nothing to fix
    aq = _tables(act)[2]
    assert aq[ORD24 + 1] == 13 and aq[ORD26 + 1] == 15
    act[ORD24 + 1], act[ORD26 + 1] = 0.9, 1.2      # headroom moves both, then the fix-up compares what came out
    aq = _tables(act, headroom=2.0)[2]             # 1.8 -> 14, 2.4 -> 13
    assert aq[ORD26 + 1] == 13 and aq[ORD24 + 1] == 13


def test_refusals_before_any_device_call():
    L = hipdrv.lib()
    err = lambda: L.yolo2_hip_last_error().decode()
    f, u = C.c_float(0), C.c_uint32(0)
    assert L.yolo2_hip_absmax_f32(0, 16, C.byref(f), C.byref(u), None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_absmax_f32(4096, 16, None, C.byref(u), None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_absmax_f32(4098, 16, C.byref(f), C.byref(u), None) == hipdrv.YOLO2_ERROR and "4-byte" in err()
    assert L.yolo2_hip_absmax_f32(4096, 0, C.byref(f), C.byref(u), None) == hipdrv.YOLO2_ERROR and "count" in err()
    assert L.yolo2_hip_calib_reset(None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_calib_frames(None, 4096, 1, None) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_calib_images_pix_host(None, None, None, None, 3, 1, 1) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_calib_stats(None, None, None, None, None) == hipdrv.YOLO2_ERROR and "null" in err()
    q = np.zeros(NCONV + 1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.yolo2_hip_calib_q_tables(None, 1.0, vp(q), vp(q), vp(q)) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_quantize_weights_int16(None, vp(q), vp(q), None, 0, None, 0, None) == hipdrv.YOLO2_ERROR and "null" in err()
    a = np.ones(NCONV + 1, np.float32)
    assert L.yolo2_hip_calib_q_from_stats(vp(a), vp(a), None, 1.0, vp(q), vp(q), vp(q)) == hipdrv.YOLO2_ERROR and "null" in err()
    assert L.yolo2_hip_calib_q_from_stats(vp(a), vp(a), vp(a), 1.0, vp(q), vp(q), None) == hipdrv.YOLO2_ERROR and "null" in err()
    with pytest.raises(ValueError):
        hipdrv.q_tables_from_stats(a[:5], a[:NCONV], a[:NCONV])


def test_calibrate_tool_usage():
    r = subprocess.run([CALIBRATE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for opt in ("--weights", "--input-dir", "--input-list", "--batch", "--headroom", "--out"):
        assert opt in r.stdout, opt
    for name in hipdrv.CalibratedModel.FILES + ("weights_reorg.bin", "bias.bin"):
        assert name in r.stdout, name
    r = subprocess.run([CALIBRATE, "--weights", "w"], capture_output=True, text=True)
    assert r.returncode == 1 and "--out" in r.stderr
    r = subprocess.run([CALIBRATE, "--out", "o", "--input-dir", "d", "--headroom", "0.5"], capture_output=True, text=True)
    assert r.returncode == 1 and "--headroom" in r.stderr


def test_written_files_read_back_and_have_the_synth_layout(tmp_path):
    """write_files puts the pad element after odd-length layers (the 425 biases of the last layer) exactly like
    SynthModel.write_files: byte-identical files from the same arrays, and read_files returns the arrays"""
    model = synth.SynthModel(seed=3, weight_q=[13] * NCONV, act_q=list(range(14, 14 - NCONV - 1, -1)))
    cal = hipdrv.CalibratedModel(model.weights_i16(), model.bias_i16(), model.weight_q, model.bias_q, model.act_q)
    want = model.write_files(str(tmp_path / "synth"), fp32=False)
    got = cal.write_files(str(tmp_path / "cal"))
    assert sorted(got) == sorted(hipdrv.CalibratedModel.FILES)
    for name in hipdrv.CalibratedModel.FILES:
        assert open(got[name], "rb").read() == open(want[name], "rb").read(), name
    assert os.path.getsize(got["bias_int16.bin"]) == 2 * (hipdrv.N_BIAS + 1)
    back = hipdrv.CalibratedModel.read_files(str(tmp_path / "cal"))
    assert np.array_equal(back.weights_i16(), cal.weights_i16()) and np.array_equal(back.bias_i16(), cal.bias_i16())
    for t in ("weight_q", "bias_q", "act_q"):
        assert np.array_equal(getattr(back, t), getattr(cal, t)) and getattr(back, t).dtype == np.int32
    with pytest.raises(ValueError):
        hipdrv.CalibratedModel(model.weights_i16()[:-1], model.bias_i16(), model.weight_q, model.bias_q, model.act_q)
