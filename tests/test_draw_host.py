"""CPU tests of the annotated frame: y2h_draw_detections_rgb24 (libyolo2_host.so), the project's statement of the reference's
yolo2_draw_detections_rgb24 (linux_app/src/yolo2_draw.c:276-369), against tests/golden/draw.npz - frames the compiled reference painted
(tests/golden/make_draw_golden.py) - and the packed font against the glyphs the reference rendered.  The GPU tests
(tests/test_gpu_draw.py) take this restatement as their expected side at the sizes the fixture does not hold."""
import ctypes as C

import numpy as np
import pytest

import orclib
from drawref import CASES, GOLD, case, host_draw, records


def test_fixture_holds_the_cases():
    assert set(CASES) >= {"glyphs0", "glyphs1", "glyphs2", "main", "nolabels", "odd33x17", "one1x1", "empty", "many845", "longlabel"}
    assert GOLD["main/frame"].shape == (64, 96, 3) and GOLD["odd33x17/frame"].shape == (17, 33, 3) and GOLD["one1x1/frame"].shape == (1, 1, 3)
    assert int(GOLD["many845/drawn"]) == 845 and int(GOLD["empty/drawn"]) == 0 and int(GOLD["nolabels/n_labels"]) == -1
    assert len(str(GOLD["longlabel/labels"][0])) > 127


@pytest.mark.parametrize("name", CASES)
def test_host_painter_equals_the_reference(name):
    frame, dets, thresh, labels, expect, drawn = case(name)
    out, n = host_draw(frame, dets, thresh, labels)
    assert n == drawn
    assert np.array_equal(out, expect)


def test_packed_font_equals_the_rendered_glyphs():
    lib = orclib.host()
    lib.y2h_draw_font.argtypes = [C.c_char_p, C.c_void_p]
    chars, words = C.create_string_buffer(64), np.zeros(64, dtype=np.uint64)
    n = lib.y2h_draw_font(chars, words.ctypes.data)
    assert n == 38 and chars.raw[:n].decode() == str(GOLD["font/chars"])
    assert np.array_equal(words[:n], GOLD["font/words"])
    bits = (words[:n, None] >> np.arange(35, dtype=np.uint64)[None, :]) & np.uint64(1)
    assert np.array_equal(bits.reshape(n, 7, 5).astype(np.uint8), GOLD["font/bitmaps"])


def test_x0_equal_x1_keeps_the_reference_rings():
    """yolo2_draw_rect_rgb24 clamps every ring again (linux_app/src/yolo2_draw.c:94-111): a box with x0 == x1 has an empty t = 1 row loop,
    and its t = 1 column loop paints the columns x0 + 1 and x0 - 1 between the rows y0 + 1 and y1 - 1 - as the compiled reference does in the
    fixture's main case, and here on a plain frame"""
    frame = np.zeros((40, 40, 3), dtype=np.uint8)
    out, n = host_draw(frame, records([0], [(.5, .5, .75, 0., .25)]), .1, None)
    assert n == 1
    box = (out == np.array([255, 30, 30], dtype=np.uint8)).all(axis=2)
    assert box[25:36, 20].all() and box[26:35, 19].all() and box[26:35, 21].all()      # x0 = x1 = 20, y0 = 25, y1 = 35
    assert not box[25, 19] and not box[35, 19] and not box[35, 21] and not box[30, 18] and not box[30, 22]


def test_null_label_entry_falls_back_to_class_n():
    """the reference hands a NULL labels[cls] to %s (undefined there); here it is the "class<cls>" of a missing list"""
    lib = orclib.host()
    lib.y2h_draw_detections_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
    frame = np.zeros((40, 120, 3), dtype=np.uint8)
    d = records([1], [(.5, .5, .75, .2, .25)])
    want, n = host_draw(frame, d, .1, None)
    out = frame.copy()
    arr = (C.c_char_p * 2)(b"person", None)
    assert lib.y2h_draw_detections_rgb24(out.ctypes.data, 120, 40, d.ctypes.data, 1, C.c_float(.1), arr, 2) == n == 1
    assert np.array_equal(out, want)
    assert not np.array_equal(out, host_draw(frame, d, .1, ["person", "x"])[0])


def test_bad_frame_is_refused():
    lib = orclib.host()
    lib.y2h_draw_detections_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
    lib.y2h_last_error.restype = C.c_char_p
    d = records([0], [(.5, .5, .5, .5, .5)])
    buf = np.zeros(12, dtype=np.uint8)
    assert lib.y2h_draw_detections_rgb24(None, 2, 2, d.ctypes.data, 1, C.c_float(.1), None, 0) == -1
    assert lib.y2h_draw_detections_rgb24(buf.ctypes.data, 0, 2, d.ctypes.data, 1, C.c_float(.1), None, 0) == -1
    assert b"draw_detections_rgb24" in lib.y2h_last_error()
