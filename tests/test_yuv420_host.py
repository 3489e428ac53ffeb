"""CPU tests of the planar YUV 4:2:0 formats (NV12, I420): y2h_yuv420_to_rgb24 (libyolo2_host.so), the host restatement of the
conversion the _pix entries apply on the GPU, against the numpy side yuv420ref.to_rgb = yuyvref.formula(to_yuyv(frame)) - the YUYV
arithmetic tests/test_yuyv_host.py pins to the compiled reference; the header's values, hipdrv's names and array shapes; the refusals
that come before any GPU call; the CLI's --video-pix-fmt.  The GPU tests (tests/test_gpu_yuv420.py) take their expected values from
the RGB24 entries fed this conversion."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orclib
import yuv420ref
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
HEADER = os.path.join(ROOT, "include", "yolo2_hip.h")
FORMATS = yuv420ref.FORMATS


def yuv420_to_rgb24(frame, fmt, w=None, h=None):
    """y2h_yuv420_to_rgb24 on a uint8 [h * 3 / 2][w] frame -> (status, uint8 [h][w][3])"""
    lib = orclib.host()
    lib.y2h_yuv420_to_rgb24.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    if w is None:
        w, h = frame.shape[1], frame.shape[0] * 2 // 3
    rgb = np.full((h, w, 3), 0xA5, dtype=np.uint8)
    return lib.y2h_yuv420_to_rgb24(frame.ctypes.data, rgb.ctypes.data, w, h, int(fmt == "nv12")), rgb


def test_the_numpy_side_places_the_planes_as_the_header_says():
    """a 4 x 2 frame by hand: Y rows, then NV12's U V pairs or I420's U plane and V plane"""
    nv12 = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [100, 200, 101, 201]], dtype=np.uint8)
    i420 = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [100, 101, 200, 201]], dtype=np.uint8)
    want = np.array([[[1, 100], [2, 200], [3, 101], [4, 201]], [[5, 100], [6, 200], [7, 101], [8, 201]]], dtype=np.uint8)
    assert np.array_equal(yuv420ref.to_yuyv(nv12, "nv12"), want)
    assert np.array_equal(yuv420ref.to_yuyv(i420, "i420"), want)
    assert np.array_equal(yuv420ref.pack(*yuv420ref.planes(nv12, "nv12"), "i420"), i420)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(2, 2), (6, 2), (2, 6), (6, 6), (34, 18)])
def test_host_conversion_equals_the_numpy_side_on_random_frames(fmt, w, h):
    frame = yuv420ref.random_frame(np.random.default_rng(w * 100 + h), w, h, fmt)
    rc, rgb = yuv420_to_rgb24(frame, fmt)
    assert rc == 0
    assert np.array_equal(rgb, yuv420ref.to_rgb(frame, fmt))


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_conversion_over_all_yuv_triples(fmt):
    """one 512 x 512 frame per Y value (yuv420ref.exhaustive_frame): every (Y, U, V) triple, each chroma pair shared by four pixels"""
    for y in range(256):
        frame = yuv420ref.exhaustive_frame(y, fmt)
        rc, rgb = yuv420_to_rgb24(frame, fmt)
        assert rc == 0
        assert np.array_equal(rgb, yuv420ref.to_rgb(frame, fmt)), y
    # the frames do cover the triples: luma y at even columns, every (u, v) block once
    yy, u, v = yuv420ref.planes(yuv420ref.exhaustive_frame(7, fmt), fmt)
    assert (yy[:, 0::2] == 7).all() and (yy[:, 1::2] == 248).all()
    assert len({(int(a), int(b)) for a, b in zip(u.reshape(-1), v.reshape(-1))}) == 65536


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_conversion_refuses_odd_sizes_and_null(fmt):
    lib = orclib.host()
    buf = np.zeros(64, dtype=np.uint8)
    for w, h in ((3, 4), (4, 3), (0, 2), (2, -2)):
        rgb = np.full((8, 8, 3), 0xA5, dtype=np.uint8)
        rc = lib.y2h_yuv420_to_rgb24(buf.ctypes.data, rgb.ctypes.data, w, h, int(fmt == "nv12"))
        assert rc != 0, (w, h)
        assert f"{w}x{h}".encode() in lib.y2h_last_error()
        assert (rgb == 0xA5).all()      # nothing written
    rgb = np.zeros((2, 2, 3), dtype=np.uint8)
    assert lib.y2h_yuv420_to_rgb24(None, rgb.ctypes.data, 2, 2, 1) != 0
    assert lib.y2h_yuv420_to_rgb24(buf.ctypes.data, None, 2, 2, 0) != 0


def test_header_and_hipdrv_name_the_formats():
    text = " ".join(re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S).split())
    for name, value in (("YOLO2_PIX_NV12", "0x3231564E"), ("YOLO2_PIX_I420", "0x32315559")):
        assert re.search(name + r" = " + value + r"\b", text), name
    assert 0x3231564E == int.from_bytes(b"NV12", "little") and 0x32315559 == int.from_bytes(b"YU12", "little")      # the V4L2 fourccs
    assert hipdrv.pix_code("nv12") == 0x3231564E and hipdrv.pix_code("i420") == 0x32315559
    assert hipdrv.PIXFMTS_420 == {"nv12": 0x3231564E, "i420": 0x32315559}
    assert [hipdrv.pix_code(k) for k in ("grey8", "rgb24", "yuyv")] == [1, 3, 0x56595559]      # the others stay
    with pytest.raises(ValueError):
        hipdrv.pix_code("nv21")
    # the header says whose formula this is
    doc = " ".join(open(HEADER).read().replace("\n *", " ").split())
    assert "own extension of the reference's formula" in doc and "swscale" in doc


@pytest.mark.parametrize("fmt", FORMATS)
def test_hipdrv_takes_arrays_of_three_half_rows(fmt):
    frame = np.zeros((72, 64), dtype=np.uint8)        # 64 x 48
    n, ptrs, ws, hs, code, keep = hipdrv._image_args([frame, np.zeros((3, 2), dtype=np.uint8)], fmt)
    assert code == hipdrv.pix_code(fmt) and list(ws) == [64, 2] and list(hs) == [48, 2]
    for bad in (np.zeros((70, 64), dtype=np.uint8),            # 70 rows are not 3 h / 2
                np.zeros((48, 64, 3), dtype=np.uint8),         # an RGB picture
                np.zeros((72, 64, 1), dtype=np.uint8)):
        with pytest.raises(ValueError):
            hipdrv._image_args([frame, bad], fmt)
        with pytest.raises(ValueError):
            hipdrv.letterbox_pix(bad, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pix_entries_refuse_odd_sizes_without_a_device(fmt):
    """argument checks that come before any GPU call"""
    L = hipdrv.lib()
    code = hipdrv.pix_code(fmt)
    name = fmt.upper().encode()
    assert L.yolo2_hip_letterbox_pix(256, 5, 4, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"even width, not 5" in L.yolo2_hip_last_error() and name in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(256, 4, 7, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"even height, not 7" in L.yolo2_hip_last_error() and name in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(0, 4, 4, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"null" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(256, 4, 4, code + 1, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"unknown pixel format" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_u8(256, 4, 4, 12, 512, 416, 416, None) == hipdrv.YOLO2_ERROR         # no channel count names the formats
    assert L.yolo2_hip_letterbox_u8(256, 4, 4, 13, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    dets = np.zeros(1, dtype=hipdrv.DET_DTYPE)
    assert L.yolo2_hip_annotate_pix(256, 4, 5, code, dets.ctypes.data_as(C.c_void_p), 0, C.c_float(0.2), None, 0, 512, None, None) == hipdrv.YOLO2_ERROR
    assert b"even height, not 5" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_annotate_pix(256, 3, 4, code, dets.ctypes.data_as(C.c_void_p), 0, C.c_float(0.2), None, 0, 512, None, None) == hipdrv.YOLO2_ERROR
    assert b"even width, not 3" in L.yolo2_hip_last_error()


# ------------------------------------------------------------------ CLI

def test_cli_help_names_the_formats():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "nv12" in r.stdout and "yuv420p" in r.stdout


@pytest.mark.parametrize("args", [["--video-pix-fmt", "nv12", "--video-width", "641"], ["--video-pix-fmt", "nv12", "--video-height", "481"],
                                  ["--video-pix-fmt", "yuv420p", "--video-width", "641"], ["--video-pix-fmt", "yuv420p", "--video-height", "481"],
                                  ["--video-pix-fmt", "i420", "--video-width", "2", "--video-height", "1"], ["--video-pix-fmt", "nv21"]])
def test_cli_refuses_odd_sizes_while_parsing(args, tmp_path):
    r = subprocess.run([CLI, "--video-raw", str(tmp_path / "none.yuv")] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "--video-pix-fmt" in r.stderr
    if "nv21" not in args:
        assert "even" in r.stderr


@pytest.mark.parametrize("args", [["--video-pix-fmt", "nv12", "--video-width", "641"], ["--video-pix-fmt", "yuv420p", "--video-height", "481"],
                                  ["--video-pix-fmt", "nv21"]])
def test_calibrate_tool_refuses_odd_sizes_while_parsing(args, tmp_path):
    tool = os.path.join(PKG, "yolov2_calibrate")
    r = subprocess.run([tool, "--out", str(tmp_path / "o"), "--video-raw", str(tmp_path / "none.yuv")] + args, capture_output=True, text=True)
    assert r.returncode != 0 and "--video-pix-fmt" in r.stderr
    r = subprocess.run([tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--video-raw" in r.stdout and "nv12" in r.stdout and "yuv420p" in r.stdout
