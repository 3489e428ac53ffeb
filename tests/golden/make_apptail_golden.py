#!/usr/bin/env python3
"""Generate tests/golden/apptail.npz from the REFERENCE's own camera-loop detection tail.

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_apptail_golden.py

The reference's camera / video loop (linux_app/src/main.c:1013-1026, :1184-1197) and its single-image mode (:827-858) turn the region
tensor into detections with linux_app/src/yolo2_postprocess.c: yolo2_forward_region_layer, yolo2_get_region_detections and
yolo2_do_nms_sort.  That tail is float throughout and rounds differently from the src/core tail that host.npz pins.  This script
compiles that translation unit from where it lies into a temporary directory OUTSIDE the repository, calls it through a few lines of
glue written into that directory, and stores only data: int16 region tensors with their Q, and per case the activated tensor as bit
patterns, the rows of dets[] in array order after the NMS, the totals and the best-class records of main.c:1039-1046.

tests/test_app_tail_host.py pins the host restatement (y2h::app_*) to it, tests/test_gpu_app_tail.py the GPU tail.

Before it writes the file the generator checks that every situation the cases are meant to hold really occurs.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_APP = "/root/reference/linux_app"
ELEMS = 425 * 169

# the glue: a region layer_t as yolo2_network.c fills it for config/yolov2.cfg, and dets[] flattened into rows
GLUE = r"""
#include <stdlib.h>
#include <string.h>
#include "yolo2_postprocess.h"
int glue_tail(float *raw, int im_w, int im_h, float thresh, float nms, float *proc, float *rows, int max_rows)
{
    layer_t l;
    memset(&l, 0, sizeof(l));
    l.type = LAYER_REGION;
    l.w = 13; l.h = 13; l.c = 425; l.out_w = 13; l.out_h = 13; l.out_c = 425; l.outputs = 425 * 169;
    l.classes = 80; l.coords = 4; l.num = 5; l.softmax = 1;
    if (yolo2_forward_region_layer(&l, raw, proc)) return -1;
    yolo2_detection_t *dets = (yolo2_detection_t *)malloc(1000 * sizeof(yolo2_detection_t));   /* main.c:842-843 */
    int n = yolo2_get_region_detections(&l, proc, im_w, im_h, 416, 416, thresh, dets, 1000);
    if (n > 0) yolo2_do_nms_sort(dets, n, l.classes, nms);                                     /* main.c:856-858 */
    for (int i = 0; i < n && i < max_rows; ++i) {
        float *r = rows + (size_t)i * 85;
        r[0] = dets[i].bbox.x; r[1] = dets[i].bbox.y; r[2] = dets[i].bbox.w; r[3] = dets[i].bbox.h; r[4] = dets[i].objectness;
        memcpy(r + 5, dets[i].prob, 80 * sizeof(float));
    }
    yolo2_free_detections(dets, n);
    free(dets);
    return n;
}
"""

# name, image w, h, thresh, nms, tensor
CASES = [
    ("low", 768, 576, 0.05, 0.45, "q9"),       # every candidate survives, bar the two injected objectness values below -10
    ("std", 768, 576, 0.25, 0.45, "q9"),
    ("tall", 300, 500, 0.25, 0.3, "q9"),
    ("square", 416, 416, 0.24, 0.45, "q9"),
    ("one1x1", 1, 1, 0.1, 0.45, "q9"),
    ("nms0", 640, 480, 0.05, 0.0, "q9"),
    ("q6_low", 640, 360, 0.02, 0.45, "q6"),
    ("q6_nms0", 416, 416, 0.004, 0.0, "q6"),
    ("q6", 1280, 720, 0.3, 0.45, "q6"),
]
SHARED = ("low", "std", "tall")              # the cases host.npz holds for the src/core tail
FLOAT_CASES = ("std", "tall", "square")      # the cases the float entry is judged on


def build_reference(tmp):
    glue = os.path.join(tmp, "glue.c")
    with open(glue, "w") as f:
        f.write(GLUE)
    so = os.path.join(tmp, "libref_apptail.so")
    # the app's own flags (linux_app/Makefile: -O2 -g); x86-64 has no fused multiply-add without -march, so nothing contracts
    subprocess.run(["gcc", "-O2", "-g", "-shared", "-fPIC", "-I" + os.path.join(REF_APP, "include"), "-o", so, glue,
                    os.path.join(REF_APP, "src", "yolo2_postprocess.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.glue_tail.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int]
    lib.glue_tail.restype = C.c_int
    return lib


def ref_tail(lib, raw_f32, w, h, thresh, nms):
    raw = np.ascontiguousarray(raw_f32, dtype=np.float32).copy()
    proc = np.zeros(ELEMS, dtype=np.float32)
    rows = np.zeros((845, 85), dtype=np.float32)
    n = lib.glue_tail(raw.ctypes.data, w, h, C.c_float(thresh), C.c_float(nms), proc.ctypes.data, rows.ctypes.data, 845)
    assert 0 <= n <= 845, n
    return proc, rows[:n].copy(), n


def best_records(rows):
    """main.c:1039-1046: per detection the best class, the first among equals; kept where its prob > 0 -> (det, cls), (prob, x, y, w, h)"""
    idx, val = [], []
    for i, r in enumerate(rows):
        bc, bp = -1, np.float32(0)
        for c in range(80):
            if r[5 + c] > bp:
                bp, bc = r[5 + c], c
        if bc >= 0:
            idx.append((i, bc))
            val.append((bp, r[0], r[1], r[2], r[3]))
    return np.array(idx, dtype=np.int32).reshape(-1, 2), np.array(val, dtype=np.float32).reshape(-1, 5)


def main():
    if not os.path.isdir(REF_APP):
        sys.exit("needs the reference tree at /root/reference")
    host = np.load(os.path.join(HERE, "host.npz"))
    refapp = np.load(os.path.join(HERE, "refapp.npz"))
    raw9 = host["detect/raw"]
    i9 = np.rint(raw9.astype(np.float64) * 512).astype(np.int64)
    assert (i9.astype(np.float32) * np.float32(2.0 ** -9) == raw9).all() and np.abs(i9).max() < 32768, "detect/raw is int16 x 2^-9"
    t = i9.astype(np.int16).reshape(5, 85, 13, 13).copy()
    assert t[:, [0, 1, 4]].max() <= 10 * 512 and t[:, [0, 1, 4]].min() >= -10 * 512, "detect/raw has nothing past +-10 today"
    # values past the sigmoid's clamp on x, y and objectness, both sides, and the clamp's edges themselves (10 is NOT clamped)
    inject = [(0, 0, 0, 0, 5121), (0, 0, 0, 1, -5121), (1, 1, 2, 3, 6000), (1, 1, 2, 4, -32768), (3, 4, 5, 5, 32767), (3, 4, 5, 6, -5121),
              (2, 0, 9, 9, 5120), (2, 1, 9, 9, -5120), (4, 4, 12, 12, 5120), (4, 4, 0, 12, -5120), (0, 4, 8, 1, 5121)]
    for a, e, y, x, v in inject:
        t[a, e, y, x] = v
    # two candidates with bit-equal inputs in different cells: equal probability in every class, the stable order decides
    t[3, :, 7, 3] = t[2, :, 6, 6]
    t[3, 0:4, 7, 3] = [100, -200, 300, -50]
    t[0, :, 11, 9] = t[0, :, 3, 4]
    # a second tensor at another final Q: the varq set's integers read at Q 6 (that set's own final Q is 9 as well: it varies the
    # inner layers' Q), so that the tables of another Q are exercised; there the values reach +-49 and the data itself hits the clamps
    varq = refapp["varq/region_raw_i16"].copy()
    assert int(refapp["varq/final_q"]) == 9
    tensors = {"q9": (t.reshape(-1), 9), "q6": (varq, 6)}
    assert {q for _, q in tensors.values()} == {9, 6}

    out = {"cases": np.array([c[0] for c in CASES])}
    # the tensors are not stored a second time: q9 is host.npz's detect/raw x 2^9 with `patch_val` at `patch_idx`, q6 is
    # refapp.npz's varq/region_raw_i16 as it is (tests/apptail_fix.py rebuilds both)
    patch = np.nonzero(t.reshape(-1) != i9)[0]
    out["tensor/q9/patch_idx"] = patch.astype(np.int32)
    out["tensor/q9/patch_val"] = t.reshape(-1)[patch]
    for name, (ti, q) in tensors.items():
        out[f"tensor/{name}/q"] = np.int32(q)
        out[f"tensor/{name}/sum"] = np.int64(ti.astype(np.int64).sum())
    res = {}
    with tempfile.TemporaryDirectory(prefix="y2_apptail_ref_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        lib = build_reference(tmp)
        for name, w, h, thresh, nms, tn in CASES:
            ti, q = tensors[tn]
            raw = ti.astype(np.float32) * np.float32(2.0 ** -q)
            proc, rows, n = ref_tail(lib, raw, w, h, thresh, nms)
            proc2, rows2, n2 = ref_tail(lib, raw, w, h, thresh, nms)
            assert n == n2 and proc.tobytes() == proc2.tobytes() and rows.tobytes() == rows2.tobytes(), "the reference is deterministic"
            # the same candidates before any suppression (nms above every IoU): which probabilities did the NMS zero?
            _, rows_pre, n_pre = ref_tail(lib, raw, w, h, thresh, 2.0)
            assert n_pre == n
            res[name] = dict(proc=proc, rows=rows, n=n, pre=rows_pre, raw=raw, thresh=np.float32(thresh), nms=np.float32(nms), w=w, h=h, tn=tn)

    # ---- does every situation occur?
    p9 = res["low"]["proc"].reshape(5, 85, 13, 13)
    for a, e, y, x, v in inject:
        want = 1.0 if v > 5120 else 0.0 if v < -5120 else None
        if want is not None:
            assert p9[a, e, y, x] == np.float32(want), (a, e, y, x, v)
        else:
            assert 0.0 < p9[a, e, y, x] < 1.0, "the clamp's edge itself is computed"
    for e in (0, 1, 4):
        vals = [v for a, ee, y, x, v in inject if ee == e]
        assert max(vals) > 5120 and min(vals) < -5120, f"entry {e}: a value past +10 and one past -10"
    pq6, iq6 = res["q6"]["proc"].reshape(5, 85, 13, 13)[:, 4], varq.reshape(5, 85, 13, 13)[:, 4]
    assert (iq6 > 640).any() and (pq6[iq6 > 640] == 1).all() and (iq6 < -640).any() and (pq6[iq6 < -640] == 0).all(), "Q 6: both clamps"
    killed = sum(1 for a, e, y, x, v in inject if e == 4 and v < 0)
    assert killed == 2 and res["low"]["n"] == 845 - killed, "at 0.05 every candidate survives but the two whose objectness was sent below -10"
    assert res["one1x1"]["n"] > 0 and res["nms0"]["n"] > 0 and res["q6_low"]["n"] > 300 and res["q6_nms0"]["n"] > 300
    for name, r in res.items():
        rows, pre = r["rows"], r["pre"]
        # the NMS only zeroes probabilities: as multisets of rows, pre >= post
        if r["n"] == 0:
            continue
        nz_pre, nz = int((pre[:, 5:] > 0).sum()), int((rows[:, 5:] > 0).sum())
        r["zeroed"] = nz_pre - nz
        r["kept"] = nz
    assert all(res[n]["zeroed"] > 0 and res[n]["kept"] > 0 for n in ("low", "nms0", "q6", "q6_low", "q6_nms0")), "suppressed and surviving probabilities"
    lo = res["low"]
    assert ((lo["pre"][:, 5:] == 0).all(axis=0)).any(), "a class whose keys are all zero"
    # ties: the copied candidates have the same objectness and class probabilities as their originals, bit for bit, so every
    # class's sort meets equal non-zero keys; the stable order keeps the earlier cell (the smaller y) in front
    ties = 0
    for name in ("low", "std"):
        pre = res[name]["pre"]
        for i in range(len(pre)):
            for j in range(i + 1, len(pre)):
                if (pre[i, 5:] > 0).any() and pre[i, 4:].tobytes() == pre[j, 4:].tobytes():
                    assert pre[i, 1] < pre[j, 1], "equal keys keep candidate order"
                    ties += 1
    assert ties >= 4, "two candidates with an equal probability in some class, in both cases"
    by_name = {c[0]: c for c in CASES}
    for name in SHARED:
        assert np.array_equal(host[f"detect/{name}/params"], np.array(by_name[name][1:5], dtype=np.float64)), name
    # against the src/core tail on the tensor WITHOUT injections (what host.npz holds): proc and rows differ
    with tempfile.TemporaryDirectory(prefix="y2_apptail_ref_") as tmp:
        lib = build_reference(tmp)
        for name in SHARED:
            r = res[name]
            proc, rows, n = ref_tail(lib, raw9, r["w"], r["h"], float(r["thresh"]), float(r["nms"]))
            assert (proc.view(np.uint32) != host["detect/proc"].view(np.uint32)).sum() > 1000, "proc differs from the src/core tail's"
            core = host[f"detect/{name}/rows"]

            def canon(a):
                a = a[a[:, 4] != 0]
                return a[np.lexsort(a.T[::-1])]
            a, b = canon(rows), canon(core)
            assert a.shape != b.shape or (a.view(np.uint32) != b.view(np.uint32)).sum() > 50, "rows differ from the src/core tail's"
    for name in FLOAT_CASES:
        r = res[name]
        th = np.float64(r["thresh"])
        p = r["proc"].reshape(5, 85, 13, 13).astype(np.float64)
        obj = p[:, 4]
        cls = obj[:, None] * p[:, 5:]
        for v in (obj, cls):
            assert (np.abs(v - th) > 1e-4 * th).all(), f"{name}: a reference value within 1e-4 of thresh"
        prf = (r["proc"].reshape(5, 85, 13, 13)[:, 4][:, None] * r["proc"].reshape(5, 85, 13, 13)[:, 5:]).astype(np.float32)
        assert (np.abs(prf.astype(np.float64) - th) > 1e-4 * th).all()

    for name, w, h, thresh, nms, tn in CASES:
        r = res[name]
        out[f"{name}/params"] = np.array([w, h, thresh, nms], dtype=np.float64)
        out[f"{name}/tensor"] = np.array(tn)
        out[f"{name}/rows"] = r["rows"].view(np.uint32)          # array order, bit patterns
        out[f"{name}/total"] = np.int32(r["n"])
        bi, bv = best_records(r["rows"])
        out[f"{name}/best_idx"] = bi
        out[f"{name}/best_val"] = bv.view(np.uint32)
    for tn in tensors:
        out[f"proc/{tn}"] = res[{"q9": "low", "q6": "q6"}[tn]]["proc"].view(np.uint32)    # the activated tensor, bit patterns
        for name, r in res.items():
            if r["tn"] == tn:
                assert r["proc"].tobytes() == out[f"proc/{tn}"].tobytes(), "proc depends on the tensor alone"
    out["float_cases"] = np.array(FLOAT_CASES)
    path = os.path.join(HERE, "apptail.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 800 * 1000, size
    print(f"wrote {path}: {size} bytes, {len(CASES)} cases; totals " + ", ".join(f"{n}={res[n]['n']}" for n in res))


if __name__ == "__main__":
    main()
