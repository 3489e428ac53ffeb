"""CPU test of the fp16 images entries' ABI: libyolo2_hip.so exports them and include/yolo2_hip.h declares them with these
argument lists (no GPU needed: the library loads without one)."""
import ctypes as C
import os
import re

import orclib
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
HEADER = os.path.join(ROOT, "include", "yolo2_hip.h")
DETS_TAIL = "int channels, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap_per_frame, int *counts"
WANT = {
    "yolo2_hip_run_images_u8_f16_host": ("int", "yolo2_hip_ctx *ctx, int split, const uint8_t *const *images, const int *widths, "
                                                "const int *heights, int channels, int n, int batch, float *region_host"),
    "yolo2_hip_run_images_u8_dets_f16": ("int", "yolo2_hip_ctx *ctx, int split, const uint8_t *const *images, const int *widths, "
                                                "const int *heights, " + DETS_TAIL),
    "yolo2_hip_multi_run_images_u8_dets_f16": ("int", "yolo2_hip_multi *m, int split, const uint8_t *const *images, const int *widths, "
                                                      "const int *heights, " + DETS_TAIL.replace("int batch", "int batch_per_device")),
    "yolo2_hip_images_layer0_kernel": ("const char *", "yolo2_hip_ctx *ctx, int split"),
}


def _declarations():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"(const char \*|int)\s*(yolo2_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(2)] = (m.group(1).strip() if m.group(1).strip() == "int" else m.group(1), " ".join(m.group(3).split()))
    return out


def test_library_exports_the_images_f16_entries():
    L = C.CDLL(hipdrv.LIB_PATH)
    for name in WANT:
        assert hasattr(L, name), name
        assert name in hipdrv.EXPORTS, name


def test_header_declares_the_images_f16_entries():
    decl = _declarations()
    for name, (ret, args) in WANT.items():
        assert name in decl, name
        assert decl[name] == (ret, args), (name, decl[name])


def test_images_layer0_kernel_is_empty_without_a_context():
    L = hipdrv.lib()
    assert L.yolo2_hip_images_layer0_kernel(None, 0) == b""
    assert L.yolo2_hip_images_layer0_kernel(None, 1) == b""


def test_letterbox_structs_are_restated_token_for_token():
    """csrc/letterbox.hpp restates kernels_pre.hpp's LetterboxArgs / LetterboxItem for the fp16 translation unit (which cannot include
    kernels_pre.hpp): the staging table the images entries write is read by both, so the two definitions must stay the same."""
    csrc = os.path.join(ROOT, "yolo-fpga-accelerator_amd", "csrc")

    def struct(path, name):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, path)).read())
        m = re.search(r"struct " + name + r" \{.*?\};", text, flags=re.S)
        assert m, (path, name)
        return " ".join(m.group(0).split())

    for name in ("LetterboxArgs", "LetterboxItem"):
        assert struct("letterbox.hpp", name) == struct("kernels_pre.hpp", name), name
