"""CPU tests of the camera loop's detection tail: y2h::app_region_forward / app_region_detections / app_nms_sort
(libyolo2_host.so), the project's statement of the reference's linux_app/src/yolo2_postprocess.c, against what that file itself
computed (tests/golden/apptail.npz, tests/golden/make_apptail_golden.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import apptail_fix as af
import orclib
from yolo2_amd import hipdrv

PKG = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", PKG, os.path.join(PKG, "libyolo2_host.so")], check=True)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", af.CASES)
def test_host_app_tail_equals_reference_bit_for_bit(name):
    c = af.case(name)
    t, q = af.tensor(c["tensor"])
    rows, totals = af.host_tail(t, q, [c["w"]], [c["h"]], c["thresh"], c["nms"])
    assert totals[0] == c["total"]
    assert np.array_equal(u32(rows[0, :c["total"]]), c["rows"]), "rows, in the reference's array order"
    assert not rows[0, c["total"]:].any()
    proc = af.host_proc(t.astype(np.float32) * np.float32(2.0 ** -q))
    assert np.array_equal(u32(proc), c["proc"])
    bi, bv = af.best_records(rows[0, :c["total"]])
    assert np.array_equal(bi, c["best_idx"]) and np.array_equal(u32(bv), c["best_val"])


def test_fixture_differs_from_the_core_tail():
    """what the src/core restatement makes of the same tensor is NOT the fixture: a tail wired to the wrong variant cannot pass"""
    c = af.case("low")
    t, q = af.tensor("q9")
    raw = t.astype(np.float32) * np.float32(2.0 ** -q)
    core = np.zeros(af.ELEMS, dtype=np.float32)
    orclib.host().y2h_region_forward(raw, core)
    assert (u32(core) != c["proc"]).sum() > 1000
    rows = np.zeros((1, 845, 85), dtype=np.float32)
    totals = np.zeros(1, dtype=np.int32)
    assert orclib.host().y2h_postprocess_batch(t.ctypes.data, 1, q, np.array([c["w"]], dtype=np.int32), np.array([c["h"]], dtype=np.int32),
                                               c["thresh"], c["nms"], 1, rows, 845, totals) == 0
    assert totals[0] != c["total"] or (u32(rows[0, :c["total"]]) != c["rows"]).any()


def test_app_batch_over_threads_equals_single_frames():
    rng = np.random.default_rng(5)
    tq9, _ = af.tensor("q9")
    tq6, _ = af.tensor("q6")
    B = 7
    region = np.stack([np.roll(tq9 if f % 2 else tq6, 169 * f) for f in range(B)]).astype(np.int16)
    region[3] = rng.integers(-3000, 3000, af.ELEMS, dtype=np.int16)
    region[5] = -32768                                     # no candidate at all
    ws = np.array([768, 300, 416, 1, 1280, 33, 640], dtype=np.int32)
    hs = np.array([576, 500, 416, 1, 720, 17, 480], dtype=np.int32)
    for thresh, nms in ((0.05, 0.45), (0.3, 0.0)):
        rows, totals = af.host_tail(region, 9, ws, hs, thresh, nms, threads=4)
        assert totals[5] == 0 and (totals[[0, 1, 2, 3, 4, 6]] > 0).all()
        for f in range(B):
            r1, t1 = af.host_tail(region[f], 9, ws[f:f + 1], hs[f:f + 1], thresh, nms, threads=1)
            assert t1[0] == totals[f] and np.array_equal(u32(r1[0]), u32(rows[f])), f


def test_unknown_tail_is_a_value_error_before_any_gpu_call():
    with pytest.raises(ValueError):
        hipdrv.run_images_dets(None, [np.zeros((4, 4, 3), dtype=np.uint8)], 1, 0.24, 0.45, tail="bogus")
    with pytest.raises(ValueError):
        hipdrv.postprocess(None, 0, 1, [4], [4], 0.24, 0.45, final_q=9, tail="App")


def test_header_flag_value():
    text = open(os.path.join(orclib.ROOT, "include", "yolo2_hip.h")).read()
    m = re.search(r"^#define\s+YOLO2_DETS_APP_TAIL\s+(\d+)\s*$", text, re.M)
    assert m and int(m.group(1)) == 2 == hipdrv.DETS_APP_TAIL
    for name in ("yolo2_hip_postprocess_int16_app", "yolo2_hip_postprocess_f32_app"):
        assert name in text and name in hipdrv.EXPORTS
