"""Helpers of the camera-loop tail's tests (tests/test_app_tail_host.py, tests/test_gpu_app_tail.py): the cases of
tests/golden/apptail.npz - what the compiled reference's linux_app/src/yolo2_postprocess.c made of two int16 region tensors
(tests/golden/make_apptail_golden.py) - and y2h_postprocess_app_batch / y2h_app_region_forward (libyolo2_host.so), the host
restatement the CPU tests pin to them and the GPU tests expect on other tensors."""
import ctypes as C
import os

import numpy as np

import orclib

GOLD = np.load(os.path.join(orclib.ROOT, "tests", "golden", "apptail.npz"))
CASES = [str(c) for c in GOLD["cases"]]
FLOAT_CASES = [str(c) for c in GOLD["float_cases"]]
ELEMS = 425 * 169
_tensors = {}


def tensor(name):
    """-> (int16 [71825], final Q).  The fixture does not store the tensors a second time: q9 is host.npz's detect/raw (exactly
    int16 x 2^-9) with the generator's injected values, q6 is refapp.npz's varq tensor, read at Q 6."""
    if name not in _tensors:
        golden = os.path.join(orclib.ROOT, "tests", "golden")
        if name == "q9":
            t = np.rint(np.load(os.path.join(golden, "host.npz"))["detect/raw"].astype(np.float64) * 512).astype(np.int16)
            t[GOLD["tensor/q9/patch_idx"]] = GOLD["tensor/q9/patch_val"]
        else:
            t = np.load(os.path.join(golden, "refapp.npz"))["varq/region_raw_i16"].astype(np.int16)
        assert t.shape == (ELEMS,) and int(t.astype(np.int64).sum()) == int(GOLD[f"tensor/{name}/sum"])
        t.setflags(write=False)
        _tensors[name] = (t, int(GOLD[f"tensor/{name}/q"]))
    return _tensors[name]


def case(name):
    """-> dict: tensor name, w, h, thresh, nms, total, rows uint32 [total][85] (array order), proc uint32 [71825],
    best_idx int32 [k][2] = (det, cls), best_val uint32 [k][5] = prob, x, y, w, h"""
    w, h, thresh, nms = GOLD[name + "/params"]
    tn = str(GOLD[name + "/tensor"])
    return dict(tensor=tn, w=int(w), h=int(h), thresh=float(thresh), nms=float(nms), total=int(GOLD[name + "/total"]), rows=GOLD[name + "/rows"],
                proc=GOLD["proc/" + tn], best_idx=GOLD[name + "/best_idx"], best_val=GOLD[name + "/best_val"])


def host():
    lib = orclib.host()
    lib.y2h_postprocess_app_batch.argtypes = lib.y2h_postprocess_batch.argtypes
    lib.y2h_postprocess_app_batch.restype = C.c_int
    lib.y2h_app_region_forward.argtypes = [C.c_void_p, C.c_void_p]
    lib.y2h_app_region_forward.restype = None
    return lib


def host_tail(region_i16, q, ws, hs, thresh, nms, threads=1):
    """y2h_postprocess_app_batch on int16 [B][71825] -> rows float32 [B][845][85] (zero behind the totals), totals int32 [B]"""
    r = np.ascontiguousarray(region_i16, dtype=np.int16).reshape(-1, ELEMS)
    B = len(r)
    rows = np.zeros((B, 845, 85), dtype=np.float32)
    totals = np.zeros(B, dtype=np.int32)
    rc = host().y2h_postprocess_app_batch(r.ctypes.data, B, int(q), np.ascontiguousarray(ws, dtype=np.int32), np.ascontiguousarray(hs, dtype=np.int32),
                                          float(thresh), float(nms), int(threads), rows, 845, totals)
    assert rc == 0, orclib.host().y2h_last_error()
    return rows, totals


def host_proc(raw_f32):
    raw = np.ascontiguousarray(raw_f32, dtype=np.float32).reshape(ELEMS)
    proc = np.zeros(ELEMS, dtype=np.float32)
    host().y2h_app_region_forward(raw.ctypes.data, proc.ctypes.data)
    return proc


def best_records(rows):
    """the best-class records of rows [n][85] (linux_app/src/main.c:1039-1046: first among equals), those with prob > 0, in array
    order -> (idx int32 [k][2], val float32 [k][5])"""
    p = rows[:, 5:]
    keep = np.nonzero((p > 0).any(axis=1))[0]
    cls = p[keep].argmax(axis=1)          # argmax returns the first of equal maxima
    val = np.concatenate([p[keep, cls][:, None], rows[keep, :4]], axis=1).astype(np.float32)
    return np.stack([keep, cls], axis=1).astype(np.int32).reshape(-1, 2), val.reshape(-1, 5)


def pair_records(rows):
    """every (row, class) pair with prob > 0 in array order, classes inner -> (idx [k][2], val [k][5])"""
    det, cls = np.nonzero(rows[:, 5:] > 0)
    val = np.concatenate([rows[det, 5 + cls][:, None], rows[det, :4]], axis=1).astype(np.float32)
    return np.stack([det, cls], axis=1).astype(np.int32).reshape(-1, 2), val.reshape(-1, 5)


def rec_arrays(dets):
    """hipdrv.DET_DTYPE records -> (idx [k][2] = det, cls; val [k][5] = prob, x, y, w, h)"""
    idx = np.stack([dets["det"], dets["cls"]], axis=1).astype(np.int32).reshape(-1, 2)
    val = np.stack([dets[f] for f in ("prob", "x", "y", "w", "h")], axis=1).astype(np.float32).reshape(-1, 5)
    return idx, val
