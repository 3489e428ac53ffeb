"""CPU tests of what the camera-loop entry makes on the device, through its host twin: csrc/draw_list.hpp's text formatter
(draw_text_glyphs: "%s %.2f" in integers, no snprintf) and record -> item arithmetic (draw_item_from_record) are ONE source for
k_draw_items, libyolo2_host.so (y2h_draw_text, y2h_draw_item) and these tests.  The expected side is Python's own "%s %.2f" of the
float32 value and the existing host painter y2h_draw_detections_rgb24 (pinned to the compiled reference by tests/test_draw_host.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orclib
from drawref import CASES, case, host_draw, records
from loopref import FONT_CHARS, draw_item, draw_text, font_words, glyphs_of, host, paint_item
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _check_probs(values):
    """label "", so the text is " <prob>"; one ctypes call per value"""
    lib = host()
    g = np.zeros(128, dtype=np.uint8)
    ptr = g.ctypes.data
    code = {i: ch for i, ch in enumerate(FONT_CHARS)}
    bad = []
    for v in values:
        n = lib.y2h_draw_text(b"", 0, C.c_float(v), ptr)
        got = "".join(code[i] for i in g[:max(n, 0)])
        want = " %.2f" % float(v)
        if got != want:
            bad.append((float(v), got, want))
            if len(bad) > 5:
                break
    assert not bad, bad


def test_two_decimals_around_every_half_hundredth():
    """every float within +-64 ulps of j / 200, j = 0..400: all the rounding boundaries of "%.2f" up to 2.0 and the exact hundredths"""
    centres = (np.arange(401, dtype=np.float64) / 200.0).astype(np.float32).view(np.uint32).astype(np.int64)
    bits = (centres[:, None] + np.arange(-64, 65)[None, :]).reshape(-1)
    bits = np.unique(bits[bits >= 0])
    _check_probs(_f32(bits.astype(np.uint32)))


def test_two_decimals_ties_zero_one_and_subnormals():
    for p, want in ((0.125, "0.12"), (0.375, "0.38"), (0.625, "0.62"), (0.875, "0.88"), (0.0, "0.00"), (1.0, "1.00")):
        n, g = draw_text(b"x", 0, p)
        assert n == 6 and "".join(FONT_CHARS[i] for i in g[:n]) == "x " + want, p
        assert (g[n:] == 0).all()
    _check_probs(_f32(np.arange(1, 2001, dtype=np.uint32)))


def test_two_decimals_on_random_bit_patterns_below_2_to_23():
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 0x4B000000, 300000, dtype=np.uint32)     # 0x4B000000 is 2^23
    _check_probs(_f32(bits))
    _check_probs(_f32(np.array([0x4AFFFFFF, 0x4AFFFFFE, 0x3F7FFFFF, 0x3F800001], dtype=np.uint32)))


def test_unprintable_probs_are_refused():
    for p in (float("inf"), float("-inf"), float("nan"), 8388608.0, 1e30):
        n, g = draw_text(b"dog", 1, p)
        assert n == -1 and (g == 0).all(), p


@pytest.mark.parametrize("length", [0, 1, 121, 122, 123, 127, 200])
def test_labels_at_the_truncation_edge(length):
    """snprintf into char[128] keeps 127 characters: a 122-character label leaves room for " 0.50" exactly, 123 cuts the last digit"""
    label = ("abcdefghijklmnopqrstuvwxyz0123456789." * 6)[:length]
    for p in (0.5, 12.25):
        want = ("%s %.2f" % (label, p))[:127]
        n, g = draw_text(label.encode(), 3, p)
        assert n == len(want) and list(g[:n]) == glyphs_of(want), (length, p)
        assert (g[n:] == 0).all()


def test_labels_with_characters_outside_the_font_and_upper_case():
    label = "Traffic-Light_#7 (x)!"
    want = "%s %.2f" % (label, 0.33)
    n, g = draw_text(label.encode(), 9, 0.33)
    assert n == len(want) and list(g[:n]) == glyphs_of(want)
    assert glyphs_of("A-z")[0] == glyphs_of("a")[0] and glyphs_of("-")[0] == 0


@pytest.mark.parametrize("cls", [0, 7, 80, 12345, 2 ** 31 - 1])
def test_missing_labels_give_class_numbers(cls):
    want = "class%d %.2f" % (cls, 0.75)
    n, g = draw_text(None, cls, 0.75)
    assert n == len(want) and list(g[:n]) == glyphs_of(want)
    # ... and so do a null label list, a class past its end and a null entry, through the item
    rec = records([cls], [[0.75, .5, .5, .2, .2]])[0]
    for labels in (None, ["a", "b"] if cls >= 2 else [], [None] * (cls + 1) if cls < 100 else None):
        rc, it = draw_item(rec, 64, 48, .24, labels)
        assert rc == 1 and int(it["nchar"]) == len(want) and list(it["text"][:len(want)]) == glyphs_of(want)


def _one_by_one(frame, dets, thresh, labels, font):
    """every record alone: what the host painter leaves of it against the Python painter of y2h_draw_item's item"""
    h, w = frame.shape[:2]
    drawn = 0
    for rec in dets:
        want, n = host_draw(frame, np.array([rec]), thresh, labels)
        rc, it = draw_item(rec, w, h, thresh, labels)
        assert rc == n, rec
        if n:
            assert np.array_equal(paint_item(frame, it, font), want), rec
            drawn += 1
        else:
            assert np.array_equal(want, frame)
    return drawn


@pytest.mark.parametrize("name", CASES)
def test_item_paints_what_the_host_painter_paints(name):
    frame, dets, thresh, labels, _expect, _drawn = case(name)
    _one_by_one(frame, dets, thresh, labels, font_words())


def test_item_at_the_extremes():
    rng = np.random.default_rng(5)
    font = font_words()
    nan, inf = float("nan"), float("inf")
    boxes = [[.9, nan, .5, .2, .2], [.9, .5, nan, .2, .2], [.9, .5, .5, nan, nan], [.9, inf, .5, .2, .2], [.9, -inf, -inf, .1, .1],
             [.9, .5, .5, inf, inf], [.9, 1e30, 1e30, 1., 1.], [.9, -1e30, .5, 3., .2], [.9, .5, .5, 1e30, 1e30],
             [.9, 3., 3., .2, .2], [.9, -2., .5, .5, .5], [.9, .5, -7., .5, .5], [.9, .5, .5, 0., 0.], [.9, .5, .5, -.4, -.4],
             [.9, .02, .02, .01, .01], [.9, .99, .99, .5, .5], [.24, .5, .5, .2, .2], [.2400001, .5, .5, .2, .2]]
    dets = records(list(rng.integers(0, 80, len(boxes))), boxes)
    names = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
    drawn = 0
    for w, h in ((64, 48), (1, 1), (7, 9), (33, 17)):
        drawn += _one_by_one(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), dets, .24, names, font)
    assert drawn >= 4 * (len(boxes) - 1)
    # a negative class is not drawn, nor is prob == thresh; a NaN prob passes the threshold test (as in the host code) and is reported
    neg = records([-1], [[.9, .5, .5, .2, .2]])[0]
    assert draw_item(neg, 64, 48, .24, names)[0] == 0
    assert draw_item(records([3], [[.5, .5, .5, .2, .2]])[0], 64, 48, .5, names)[0] == 0
    for p in (nan, inf, 8388608.0):
        assert draw_item(records([3], [[p, .5, .5, .2, .2]])[0], 64, 48, .24, names)[0] == -1
    assert draw_item(records([3], [[-inf, .5, .5, .2, .2]])[0], 64, 48, .24, names)[0] == 0


def test_abi_surface(tmp_path):
    L = C.CDLL(hipdrv.LIB_PATH)
    for name in ("yolo2_hip_loop_images_pix", "yolo2_hip_multi_loop_images_pix", "yolo2_hip_loop_last_info"):
        assert hasattr(L, name), name
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yolo2_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %zu %zu %zu\\n", YOLO2_LOOP_INT16, YOLO2_LOOP_FP16, YOLO2_LOOP_F32TOL,\n'
                   '    YOLO2_LOOP_OUT_RGB24, YOLO2_LOOP_OUT_JPEG, sizeof(yolo2_hip_loop_info_t), offsetof(yolo2_hip_loop_info_t, items_built),\n'
                   '    offsetof(yolo2_hip_loop_info_t, items_kernel)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [0, 1, 2, 0, 1, C.sizeof(hipdrv.LoopInfo), hipdrv.LoopInfo.items_built.offset, hipdrv.LoopInfo.items_kernel.offset]
    assert C.sizeof(hipdrv.LoopInfo) == 72 and hipdrv.LOOP_PRECISIONS == {"int16": 0, "fp16": 1, "fp32fast": 2}


def test_cli_refuses_loop_gpu_without_its_companions(tmp_path):
    cli = os.path.join(PKG, "yolov2_detect")
    (tmp_path / "list.txt").write_text("nothing.ppm\n")
    base = [cli, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names"),
            "--weights", str(tmp_path), "--input-list", str(tmp_path / "list.txt"), "--loop-gpu"]
    for extra in ([], ["--annotate-gpu"], ["--save-annotated-dir", str(tmp_path / "out")],
                  ["--annotate-gpu", "--save-annotated-dir", str(tmp_path / "out"), "--post", "host"]):
        res = subprocess.run(base + extra, capture_output=True, text=True, cwd=str(tmp_path))
        assert res.returncode != 0 and "--loop-gpu joins" in res.stderr and "--annotate-gpu" in res.stderr, (extra, res.stderr[-500:])
        assert not (tmp_path / "out").exists()
    # a single-image run has no chunks to join
    res = subprocess.run(base[:7] + ["--loop-gpu", "--annotate-gpu", "--save-annotated-dir", str(tmp_path / "out"), "x.ppm"], capture_output=True,
                         text=True, cwd=str(tmp_path))
    assert res.returncode != 0 and "--loop-gpu joins" in res.stderr
