"""Helpers of the annotated-frame tests (tests/test_draw_host.py, tests/test_gpu_draw.py): the cases of tests/golden/draw.npz - frames,
records, labels and what the compiled reference's yolo2_draw_detections_rgb24 painted (tests/golden/make_draw_golden.py) - and
y2h_draw_detections_rgb24 (libyolo2_host.so), the host restatement the CPU tests pin to them and the GPU tests expect at other sizes."""
import ctypes as C
import os

import numpy as np

import orclib
from yolo2_amd import hipdrv

GOLD = np.load(os.path.join(orclib.ROOT, "tests", "golden", "draw.npz"))
CASES = [str(c) for c in GOLD["cases"]]


def records(cls, box, frame=0):
    """cls int [n], box float [n][5] = prob, x, y, w, h -> yolo2_hip_det records (hipdrv.DET_DTYPE)"""
    d = np.zeros(len(cls), dtype=hipdrv.DET_DTYPE)
    box = np.asarray(box, dtype=np.float32).reshape(len(cls), 5)
    d["frame"], d["det"], d["cls"] = frame, np.arange(len(cls)), np.asarray(cls, dtype=np.int32)
    for k, f in enumerate(("prob", "x", "y", "w", "h")):
        d[f] = box[:, k]
    return d


def case(name):
    """-> frame uint8 [h][w][3], records, thresh, labels (list of str, or None), expected frame, expected return value"""
    frame = GOLD[name + "/frame"]
    n_labels = int(GOLD[name + "/n_labels"])
    labels = None if n_labels < 0 else [str(s) for s in GOLD[name + "/labels"]][:n_labels]
    expect = np.where(GOLD[name + "/painted"][:, :, None], GOLD[name + "/paint"], frame)
    return frame, records(GOLD[name + "/cls"], GOLD[name + "/box"]), float(GOLD[name + "/thresh"]), labels, expect, int(GOLD[name + "/drawn"])


def host_draw(frame, dets, thresh, labels):
    """y2h_draw_detections_rgb24 on a copy of frame -> (painted frame, records drawn)"""
    lib = orclib.host()
    lib.y2h_draw_detections_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
    lib.y2h_draw_detections_rgb24.restype = C.c_int
    out = np.ascontiguousarray(frame, dtype=np.uint8).copy()
    h, w = out.shape[:2]
    dets = np.ascontiguousarray(dets, dtype=hipdrv.DET_DTYPE)
    arr, n_labels = None, 0
    if labels is not None:
        arr, n_labels = (C.c_char_p * max(len(labels), 1))(*[s.encode() for s in labels]), len(labels)
    return out, lib.y2h_draw_detections_rgb24(out.ctypes.data, w, h, dets.ctypes.data if len(dets) else None, len(dets), C.c_float(thresh), arr, n_labels)
