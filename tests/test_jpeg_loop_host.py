"""CPU tests of the camera loop from JPEG streams (yolo2_hip_loop_images_jpeg, yolo2_hip_multi_loop_images_jpeg,
yolo2_hip_multi_run_images_jpeg_dets): the declarations, their bindings and index lines, and every refusal that needs no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import jpegdec_cases as jc
import orclib
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
C = hipdrv.C
HEADER = open(os.path.join(ROOT, "include", "yolo2_hip.h")).read()

LOOP_TAIL = ("float thresh, float nms, int flags, yolo2_hip_det *dets, int cap_per_frame, int *counts, int *final_q, "
             "const char *const *labels, int n_labels, int out_format, int quality, uint8_t *const *out, const size_t *caps, "
             "size_t *out_sizes, int *drawn, int *status")
STREAMS = "int precision, const uint8_t *const *streams, const size_t *sizes, int *widths, int *heights, int n, "
WANT = {
    "yolo2_hip_loop_images_jpeg": "yolo2_hip_ctx *ctx, " + STREAMS + "int batch, " + LOOP_TAIL,
    "yolo2_hip_multi_loop_images_jpeg": "yolo2_hip_multi *m, " + STREAMS + "int batch_per_device, " + LOOP_TAIL,
    "yolo2_hip_multi_run_images_jpeg_dets": "yolo2_hip_multi *m, " + STREAMS + "int batch_per_device, float thresh, float nms, int flags, "
                                            "yolo2_hip_det *dets, int cap_per_frame, int *counts, int *final_q, int *status",
}


def declared(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/yolo2_hip.h"
    return re.sub(r"\s+", " ", m.group(1)).strip()


@pytest.mark.parametrize("name", sorted(WANT))
def test_symbol_is_declared_bound_exported_and_indexed(name):
    assert declared(name) == WANT[name]
    assert name in hipdrv.EXPORTS and hasattr(C.CDLL(hipdrv.LIB_PATH), name)
    assert len(getattr(hipdrv.lib(), name).argtypes) == WANT[name].count(",") + 1
    index = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"`" + name + r"`", index), f"{name} is not in INTEGRATION.md's index (tools/abi_index.py)"


def test_loop_info_struct_and_tables_are_unchanged():
    assert C.sizeof(hipdrv.LoopInfo) == 72
    assert hipdrv.LOOP_PRECISIONS == {"int16": 0, "fp16": 1, "fp32fast": 2}
    assert hipdrv.PIXFMTS == {"grey8": 1, "rgb24": 3, "yuyv": 0x56595559}


def _args(handle=None, multi=False):
    ok = jc.stream("jpg/base_420")
    keep = C.create_string_buffer(ok, len(ok))
    n = 1
    ptrs, sizes = (C.c_void_p * n)(C.addressof(keep)), (C.c_size_t * n)(len(ok))
    ws, hs, counts, drawn, status = ((C.c_int * n)(-5) for _ in range(5))
    dets = np.zeros((n, 8), dtype=hipdrv.DET_DTYPE)
    out = np.full(97 * 61 * 3, 0xA5, dtype=np.uint8)
    optrs, caps, osizes = (C.c_void_p * n)(out.ctypes.data), (C.c_size_t * n)(out.size), (C.c_size_t * n)(77)
    a = [handle, 0, ptrs, sizes, ws, hs, n, 1, 0.2, 0.45, hipdrv.DETS_BEST_CLASS, dets.ctypes.data_as(C.c_void_p), 8, counts, None, None, 0, 0, 80,
         optrs, caps, osizes, drawn, status]
    return a, (keep, out, ws, hs, counts, drawn, status, osizes, dets)


@pytest.mark.parametrize("name", ["yolo2_hip_loop_images_jpeg", "yolo2_hip_multi_loop_images_jpeg"])
def test_null_context_and_null_arguments_are_refused_without_a_device(name):
    L = hipdrv.lib()
    a, keep = _args()
    assert getattr(L, name)(*a) == hipdrv.YOLO2_ERROR and b"null argument" in L.yolo2_hip_last_error()
    out, ws, counts, osizes = keep[1], keep[2], keep[4], keep[7]
    assert (out == 0xA5).all() and ws[0] == -5 and counts[0] == -5 and osizes[0] == 77


def test_null_arguments_of_the_multi_records_entry():
    L = hipdrv.lib()
    a, keep = _args()
    assert L.yolo2_hip_multi_run_images_jpeg_dets(*(a[:15] + [a[23]])) == hipdrv.YOLO2_ERROR and b"null argument" in L.yolo2_hip_last_error()


def test_python_refuses_int8_before_any_call():
    with pytest.raises(ValueError, match="no int8 form"):
        hipdrv.loop_jpegs(None, [jc.stream("jpg/base_420")], precision="int8")
    with pytest.raises(ValueError, match="precision must be one of"):
        hipdrv.loop_jpegs(None, [jc.stream("jpg/base_420")], precision="fp64")
    with pytest.raises(ValueError, match="no int8 form"):
        hipdrv.run_jpegs_dets(None, [jc.stream("jpg/base_420")], 1, 0.2, 0.45, precision="int8", multi=True)
    for cls in (hipdrv.Yolo2Hip, hipdrv.Yolo2HipMulti):
        assert callable(getattr(cls, "loop_jpegs"))
    assert callable(hipdrv.Yolo2HipMulti.run_jpegs_dets)


def _cli(args, cwd):
    return subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                           os.path.join(PKG, "config", "coco.names")] + args, capture_output=True, text=True, cwd=str(cwd),
                          env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_accepts_decode_gpu_with_the_loop_and_keeps_its_other_refusals(tmp_path):
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "a.jpg").write_bytes(jc.stream("jpg/base_420"))
    base = ["--weights", str(tmp_path / "none"), "--input-dir", str(tmp_path / "in"), "--post", "gpu", "--decode", "gpu"]
    r = _cli(base + ["--decode-split", "128", "--loop-gpu", "--annotate-gpu", "--save-annotated-dir", str(tmp_path / "d")], tmp_path)
    # past the argument checks: it fails later, for its missing weights (without a GPU: for the missing device)
    assert r.returncode != 0 and "--decode gpu decodes" not in r.stderr and "--loop-gpu joins" not in r.stderr, r.stderr
    assert "streaming (dir)" in r.stdout and r.stderr.startswith("Fatal error: ")
    r = _cli(base + ["--save-annotated-dir", str(tmp_path / "d")], tmp_path)
    assert r.returncode != 0 and "--decode gpu decodes" in r.stderr
    r = _cli(base + ["--annotate-gpu", "--save-annotated-dir", str(tmp_path / "d")], tmp_path)
    assert r.returncode != 0 and "--decode gpu decodes" in r.stderr
    r = _cli(base + ["--precision", "int8", "--loop-gpu", "--annotate-gpu", "--save-annotated-dir", str(tmp_path / "d")], tmp_path)
    assert r.returncode != 0 and "have no int8 form" in r.stderr
