"""CPU tests of the YUYV camera format: y2h_yuyv_to_rgb24 (libyolo2_host.so), the project's statement of the reference's
yolo2_yuyv_to_rgb24 (linux_app/src/yolo2_v4l2.c:328-374), against tests/golden/yuyv.npz - frames the compiled reference converted
and the sha256 of its output over all 2^24 (Y, U, V) triples (tests/golden/make_yuyv_golden.py) -; the ABI of the _pix entries; the
CLI's --video-pix-fmt.  The GPU tests (tests/test_gpu_yuyv.py) take their expected values from the RGB entries fed this conversion."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv
from yuyvref import exhaustive_frame, formula

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
HEADER = os.path.join(ROOT, "include", "yolo2_hip.h")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "yuyv.npz"))
FRAMES = sorted(k[:-5] for k in GOLD.files if k.endswith("/yuyv"))


def yuyv_to_rgb24(yuyv):
    """y2h_yuyv_to_rgb24 on a uint8 [h][w][2] frame -> (status, uint8 [h][w][3])"""
    lib = orclib.host()
    lib.y2h_yuyv_to_rgb24.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    yuyv = np.ascontiguousarray(yuyv, dtype=np.uint8)
    h, w = yuyv.shape[:2]
    rgb = np.full((h, w, 3), 0xA5, dtype=np.uint8)
    return lib.y2h_yuyv_to_rgb24(yuyv.ctypes.data, rgb.ctypes.data, w, h), rgb


def test_fixture_covers_the_sizes_and_both_clamps():
    assert {GOLD[n + "/yuyv"].shape[:2][::-1] for n in FRAMES} >= {(2, 1), (2, 2), (6, 5), (64, 48)}
    r = GOLD["random_32x24/rgb"]
    assert (r == 0).any(axis=(0, 1)).all() and (r == 255).any(axis=(0, 1)).all()


@pytest.mark.parametrize("name", FRAMES)
def test_host_conversion_equals_the_reference_frames(name):
    rc, rgb = yuyv_to_rgb24(GOLD[name + "/yuyv"])
    assert rc == 0
    assert np.array_equal(rgb, GOLD[name + "/rgb"])
    assert np.array_equal(formula(GOLD[name + "/yuyv"]), GOLD[name + "/rgb"])    # the numpy statement the GPU tests use


def test_host_conversion_over_all_yuv_triples():
    """for y in 0..255 one 512 x 256 frame whose pairs are (y, u, 255 - y, v), u = row, v = pair in the row; the 256 outputs hashed in order"""
    sha, sha_np = hashlib.sha256(), hashlib.sha256()
    for y in range(256):
        rc, rgb = yuyv_to_rgb24(exhaustive_frame(y))
        assert rc == 0
        sha.update(rgb.tobytes())
        sha_np.update(formula(exhaustive_frame(y)).tobytes())
    want = GOLD["exhaustive_sha256"].tobytes().hex()
    assert want == "aa952659e845ecb743186daf48be932e6c6d584a072f2d367ef85242d18d2b4f"
    assert sha.hexdigest() == want
    assert sha_np.hexdigest() == want


def test_host_conversion_refuses_an_odd_width():
    rc, rgb = yuyv_to_rgb24(np.zeros((4, 3, 2), dtype=np.uint8))
    assert rc != 0
    assert b"3x4" in orclib.host().y2h_last_error()
    assert (rgb == 0xA5).all()      # nothing written
    lib = orclib.host()
    assert lib.y2h_yuyv_to_rgb24(None, rgb.ctypes.data, 2, 2) != 0


# ------------------------------------------------------------------ ABI

IMAGES = "const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, "
DETS = "float thresh, float nms, int flags, yolo2_hip_det *dets, int cap_per_frame, int *counts"
WANT = {
    "yolo2_hip_letterbox_pix": "uint64_t image_dev, int w, int h, int pixfmt, uint64_t frame_dev, int net_w, int net_h, void *stream",
    "yolo2_hip_run_images_pix_host": "yolo2_hip_ctx *ctx, " + IMAGES + "int batch, int16_t *region_host, int *final_q",
    "yolo2_hip_run_images_pix_dets": "yolo2_hip_ctx *ctx, " + IMAGES + "int batch, " + DETS + ", int *final_q",
    "yolo2_hip_run_images_pix_f16_host": "yolo2_hip_ctx *ctx, int split, " + IMAGES + "int batch, float *region_host",
    "yolo2_hip_run_images_pix_dets_f16": "yolo2_hip_ctx *ctx, int split, " + IMAGES + "int batch, " + DETS,
    "yolo2_hip_multi_run_images_pix_dets": "yolo2_hip_multi *m, " + IMAGES + "int batch_per_device, " + DETS + ", int *final_q",
    "yolo2_hip_multi_run_images_pix_dets_f16": "yolo2_hip_multi *m, int split, " + IMAGES + "int batch_per_device, " + DETS,
    "yolo2_hip_multi_run_images_pix_host": "yolo2_hip_multi *m, " + IMAGES + "int batch_per_device, int16_t *region_host, int *final_q",
}


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_library_exports_the_pix_entries():
    L = C.CDLL(hipdrv.LIB_PATH)
    for name in WANT:
        assert hasattr(L, name), name
        assert name in hipdrv.EXPORTS, name


def test_header_declares_the_pix_entries():
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"int\s+(yolo2_hip_\w+)\s*\(([^)]*)\)\s*;", _header())}
    for name, args in WANT.items():
        assert decl.get(name) == args, (name, decl.get(name))
        # the u8 entry it mirrors: the same list with `int channels`
        u8 = name.replace("_pix", "_u8")
        assert decl[u8] == args.replace("int pixfmt", "int channels"), u8


def test_header_has_the_pixel_format_values():
    text = " ".join(_header().split())
    for name, value in (("YOLO2_PIX_GREY8", "1"), ("YOLO2_PIX_RGB24", "3"), ("YOLO2_PIX_YUYV", "0x56595559")):
        assert re.search(name + r" = " + value + r"\b", text), name
    assert 0x56595559 == int.from_bytes(b"YUYV", "little")      # the V4L2 fourcc
    assert hipdrv.PIXFMTS == {"grey8": 1, "rgb24": 3, "yuyv": 0x56595559}


def test_pix_entries_refuse_bad_formats_without_a_device():
    """argument checks that come before any GPU call"""
    L = hipdrv.lib()
    assert L.yolo2_hip_letterbox_pix(256, 4, 4, 2, 512, 416, 416, None) == hipdrv.YOLO2_ERROR       # 2 is not a pixfmt
    assert b"unknown pixel format" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(256, 5, 4, hipdrv.PIXFMTS["yuyv"], 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"even width, not 5" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_u8(256, 4, 4, 2, 512, 416, 416, None) == hipdrv.YOLO2_ERROR         # channels == 2 stays an error
    with pytest.raises(ValueError):
        hipdrv.letterbox_pix(np.zeros((4, 4, 3), dtype=np.uint8), "yuyv")
    with pytest.raises(ValueError):
        hipdrv.letterbox_pix(np.zeros((4, 4, 2), dtype=np.uint8), "uyvy")


# ------------------------------------------------------------------ CLI

def test_cli_help_names_the_pixel_format_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--video-pix-fmt" in r.stdout and "yuyv422" in r.stdout


@pytest.mark.parametrize("args", [["--video-pix-fmt", "nv12"], ["--video-pix-fmt", "yuyv422", "--video-width", "641"]])
def test_cli_refuses_a_bad_pixel_format_while_parsing(args, tmp_path):
    r = subprocess.run([CLI, "--video-raw", str(tmp_path / "none.yuv")] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "--video-pix-fmt" in r.stderr
