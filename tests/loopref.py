"""Helpers of the camera-loop tests (tests/test_loop_host.py, tests/test_gpu_loop.py): the DrawItem layout of csrc/draw_list.hpp, the
host twin of k_draw_items (y2h_draw_text / y2h_draw_item in libyolo2_host.so) and a painter of ONE item written here in Python, so that
an item can be held against what y2h_draw_detections_rgb24 paints for its record."""
import ctypes as C

import numpy as np

import orclib
from yolo2_amd import hipdrv

FONT_CHARS = " .0123456789abcdefghijklmnopqrstuvwxyz"
ITEM_DTYPE = np.dtype([("ring", np.int32, (2, 4)), ("tag", np.int32, 4), ("gx", np.int32), ("gy", np.int32), ("nchar", np.int32),
                       ("box_rgb", np.uint32), ("text_rgb", np.uint32), ("ext", np.int32, 4), ("text", np.uint8, 128)])


def host():
    lib = orclib.host()
    lib.y2h_draw_text.argtypes = [C.c_char_p, C.c_int, C.c_float, C.c_void_p]
    lib.y2h_draw_text.restype = C.c_int
    lib.y2h_draw_item.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
    lib.y2h_draw_item.restype = C.c_int
    lib.y2h_draw_item_size.restype = C.c_size_t
    lib.y2h_draw_font.argtypes = [C.c_char_p, C.c_void_p]
    return lib


def glyph_index(ch: str) -> int:
    """a character's glyph: upper case uses lower case's, anything outside the font is the blank"""
    return max(FONT_CHARS.find(ch.lower()), 0) if ch.isascii() else 0


def glyphs_of(text: str):
    return [glyph_index(c) for c in text]


def draw_text(label, cls, prob):
    """y2h_draw_text -> (return value, glyph indices [128])"""
    g = np.full(128, 0xEE, dtype=np.uint8)
    n = host().y2h_draw_text(None if label is None else label, cls, C.c_float(prob), g.ctypes.data)
    return n, g


def _label_array(labels):
    if labels is None:
        return None, 0
    return (C.c_char_p * max(len(labels), 1))(*[None if s is None else (s.encode() if isinstance(s, str) else s) for s in labels]), len(labels)


def draw_item(rec, w, h, thresh, labels):
    """y2h_draw_item on one record (a DET_DTYPE element) -> (return value, the item as an ITEM_DTYPE scalar)"""
    assert host().y2h_draw_item_size() == ITEM_DTYPE.itemsize
    r = np.ascontiguousarray(rec, dtype=hipdrv.DET_DTYPE).reshape(1)
    it = np.zeros(1, dtype=ITEM_DTYPE)
    arr, n_labels = _label_array(labels)
    rc = host().y2h_draw_item(r.ctypes.data, w, h, C.c_float(thresh), arr, n_labels, it.ctypes.data)
    return rc, it[0]


def font_words():
    chars = C.create_string_buffer(64)
    words = np.zeros(64, dtype=np.uint64)
    n = host().y2h_draw_font(chars, words.ctypes.data)
    assert chars.raw[:n].decode() == FONT_CHARS
    return [int(x) for x in words[:n]]


def paint_item(frame, it, font):
    """what the painter leaves of ONE item (yolo2_draw.c's order: ring 0, ring 1, the tag's rectangle, the glyphs, every pixel
    bounds-checked), on a copy of frame"""
    out = frame.copy()
    h, w = out.shape[:2]
    rgb = lambda c: (int(c) & 255, (int(c) >> 8) & 255, (int(c) >> 16) & 255)

    def span(x0, y0, x1, y1, c):   # inclusive, clipped to the image
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
        if x0 <= x1 and y0 <= y1:
            out[y0:y1 + 1, x0:x1 + 1] = c
    box, text = rgb(it["box_rgb"]), rgb(it["text_rgb"])
    for r in it["ring"]:
        x0, y0, x1, y1 = (int(v) for v in r)
        span(x0, y0, x1, y0, box); span(x0, y1, x1, y1, box); span(x0, y0, x0, y1, box); span(x1, y0, x1, y1, box)
    span(*(int(v) for v in it["tag"]), box)
    for k in range(int(it["nchar"])):
        g = font[int(it["text"][k])]
        for b in range(35):
            if (g >> b) & 1:
                px, py = int(it["gx"]) + k * 12 + (b % 5) * 2, int(it["gy"]) + (b // 5) * 2
                span(px, py, px + 1, py + 1, text)
    return out
