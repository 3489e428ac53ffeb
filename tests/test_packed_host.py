"""CPU tests of the packed RGB formats (BGR24, RGBA32, BGRA32): y2h_packed_to_rgb24 (libyolo2_host.so), the host restatement of the
byte reorder the _pix entries apply where they fetch a pixel, against the numpy side packedref.to_rgb; the header's values, hipdrv's
names and array shapes; the refusals that come before any GPU call; the CLI's --video-pix-fmt.  The GPU tests
(tests/test_gpu_packed.py) take their expected values from the RGB24 entries fed this reorder."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orclib
import packedref
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
CALIBRATE = os.path.join(PKG, "yolov2_calibrate")
HEADER = os.path.join(ROOT, "include", "yolo2_hip.h")
FORMATS = packedref.FORMATS
CODES = {"bgr24": 0x33524742, "rgba32": 0x34324241, "bgra32": 0x34325241}
SHAPES = [(1, 1), (2, 2), (5, 3), (3, 5), (3, 1000), (1000, 3), (33, 17)]      # (w, h): the random frames of the GPU tests


def packed_to_rgb24(frame, code, w=None, h=None):
    """y2h_packed_to_rgb24 on a uint8 [h][w][bpp] frame -> (status, uint8 [h][w][3])"""
    lib = orclib.host()
    lib.y2h_packed_to_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    if w is None:
        h, w = frame.shape[:2]
    rgb = np.full((max(h, 1), max(w, 1), 3), 0xA5, dtype=np.uint8)
    return lib.y2h_packed_to_rgb24(frame.ctypes.data, w, h, code, rgb.ctypes.data), rgb


def test_the_numpy_side_places_the_bytes_as_the_header_says():
    """a 2 x 1 frame by hand: B G R at 3x; R G B X and B G R X at 4x"""
    rgb = np.array([[[10, 20, 30], [40, 50, 60]]], dtype=np.uint8)
    frames = {"bgr24": [30, 20, 10, 60, 50, 40], "rgba32": [10, 20, 30, 7, 40, 50, 60, 9], "bgra32": [30, 20, 10, 7, 60, 50, 40, 9]}
    for fmt in FORMATS:
        frame = np.array(frames[fmt], dtype=np.uint8).reshape(1, 2, packedref.BPP[fmt])
        assert np.array_equal(packedref.to_rgb(frame, fmt), rgb), fmt
        assert np.array_equal(packedref.from_rgb(rgb, fmt, np.array([[7, 9]], dtype=np.uint8)), frame), fmt
        for k in range(3):      # the header's rule: byte k of pixel x is row[x * bpp + (swap ? 2 - k : k)]
            assert packedref.ORDER[fmt][k] == (2 - k if packedref.SWAP[fmt] else k)
            assert frame[0, 1, packedref.ORDER[fmt][k]] == rgb[0, 1, k]
    # the same picture in every format, the fourth byte random
    a, b, c = (packedref.random_frame(np.random.default_rng(5), 5, 3, fmt) for fmt in FORMATS)
    assert np.array_equal(packedref.to_rgb(a, "bgr24"), packedref.to_rgb(b, "rgba32")) and np.array_equal(packedref.to_rgb(a, "bgr24"), packedref.to_rgb(c, "bgra32"))
    assert len(np.unique(b[..., 3])) > 4 and np.array_equal(b[..., 3], c[..., 3])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_host_reorder_equals_the_numpy_side(fmt, w, h):
    frame = packedref.random_frame(np.random.default_rng(w * 10007 + h), w, h, fmt)
    rc, rgb = packed_to_rgb24(frame, CODES[fmt])
    assert rc == 0
    assert np.array_equal(rgb, packedref.to_rgb(frame, fmt))
    if packedref.BPP[fmt] == 4:      # the fourth byte is not read into the result
        other = frame.copy()
        other[..., 3] ^= 0xff
        assert np.array_equal(packed_to_rgb24(other, CODES[fmt])[1], rgb)


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_reorder_refuses_null_bad_sizes_and_unknown_formats(fmt):
    lib = orclib.host()
    buf = np.zeros(64, dtype=np.uint8)
    for w, h in ((0, 2), (2, -2)):
        rgb = np.full((8, 8, 3), 0xA5, dtype=np.uint8)
        assert lib.y2h_packed_to_rgb24(buf.ctypes.data, w, h, CODES[fmt], rgb.ctypes.data) != 0, (w, h)
        assert f"{w}x{h}".encode() in lib.y2h_last_error()
        assert (rgb == 0xA5).all()      # nothing written
    rgb = np.full((2, 2, 3), 0xA5, dtype=np.uint8)
    assert lib.y2h_packed_to_rgb24(None, 2, 2, CODES[fmt], rgb.ctypes.data) != 0
    assert lib.y2h_packed_to_rgb24(buf.ctypes.data, 2, 2, CODES[fmt], None) != 0
    for code in (0, 2, 3, 7, 0x56595559, 0x59565955, 0x3231564E, CODES[fmt] ^ 0x100):      # RGB24 and the YUV formats are not this function's
        assert lib.y2h_packed_to_rgb24(buf.ctypes.data, 2, 2, code, rgb.ctypes.data) != 0, hex(code)
        assert b"unknown pixel format" in lib.y2h_last_error()
    assert (rgb == 0xA5).all()


def test_header_and_hipdrv_name_the_formats():
    text = " ".join(re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S).split())
    for name, value in (("YOLO2_PIX_BGR24", "0x33524742"), ("YOLO2_PIX_RGBA32", "0x34324241"), ("YOLO2_PIX_BGRA32", "0x34325241"),
                        ("YOLO2_LOOP_OUT_BGR24", "0x33524742")):
        assert re.search(name + r" = " + value + r"\b", text), name
    assert [int.from_bytes(s, "little") for s in (b"BGR3", b"AB24", b"AR24")] == [CODES[f] for f in FORMATS]      # the V4L2 fourccs
    assert hipdrv.PIXFMTS_PACKED == CODES
    assert [hipdrv.pix_code(f) for f in FORMATS] == [CODES[f] for f in FORMATS]
    assert hipdrv.LOOP_OUT_BGR24 == 0x33524742 and (hipdrv.LOOP_OUT_RGB24, hipdrv.LOOP_OUT_JPEG) == (0, 1)
    # the other tables stay
    assert hipdrv.PIXFMTS == {"grey8": 1, "rgb24": 3, "yuyv": 0x56595559} and hipdrv.PIXFMTS_420 == {"nv12": 0x3231564E, "i420": 0x32315559}
    for name in ("uyvy", "nv21", "rgba", "bgr"):
        with pytest.raises(ValueError):
            hipdrv.pix_code(name)
    doc = " ".join(open(HEADER).read().replace("\n *", " ").split())
    assert "no result of any entry depends on the fourth byte" in doc and "y2h_packed_to_rgb24" in doc


@pytest.mark.parametrize("fmt", FORMATS)
def test_hipdrv_takes_arrays_of_the_formats_last_dimension(fmt):
    bpp = packedref.BPP[fmt]
    frame = np.zeros((48, 64, bpp), dtype=np.uint8)
    n, ptrs, ws, hs, code, keep = hipdrv._image_args([frame, np.zeros((1, 2, bpp), dtype=np.uint8)], fmt)
    assert code == CODES[fmt] and list(ws) == [64, 2] and list(hs) == [48, 1]
    for bad in (np.zeros((48, 64, 7 - bpp), dtype=np.uint8),      # the other width of pixel
                np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64, 2), dtype=np.uint8)):
        with pytest.raises(ValueError):
            hipdrv._image_args([frame, bad], fmt)
        with pytest.raises(ValueError):
            hipdrv.letterbox_pix(bad, fmt)
        with pytest.raises(ValueError):
            hipdrv.packed_to_rgb24_host(bad, fmt)
    with pytest.raises(ValueError):
        hipdrv.packed_to_rgb24_host(np.zeros((4, 4, 3), dtype=np.uint8), "rgb24")
    pic = packedref.random_frame(np.random.default_rng(3), 7, 5, fmt)
    assert np.array_equal(hipdrv.packed_to_rgb24_host(pic, fmt), packedref.to_rgb(pic, fmt))


def test_loop_out_order_is_checked_before_any_call():
    frame = np.zeros((4, 4, 3), dtype=np.uint8)
    for call in (hipdrv.loop_images, hipdrv.loop_jpegs):
        with pytest.raises(ValueError, match="jpeg_quality"):
            call(None, [frame], jpeg_quality=80, out_order="bgr")
        with pytest.raises(ValueError, match="out_order"):
            call(None, [frame], out_order="gbr")


@pytest.mark.parametrize("fmt", FORMATS)
def test_pix_entries_refuse_before_any_device_call(fmt):
    """argument checks that come before any GPU call"""
    L = hipdrv.lib()
    code = CODES[fmt]
    name = fmt.upper().encode()
    assert L.yolo2_hip_letterbox_pix(0, 4, 4, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"null" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(256, 0, 4, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"bad image geometry" in L.yolo2_hip_last_error()
    for w, h in ((2, 1000), (1000, 2)):
        assert L.yolo2_hip_letterbox_pix(256, w, h, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
        assert b"aspect too extreme" in L.yolo2_hip_last_error()
    dets = np.zeros(1, dtype=hipdrv.DET_DTYPE)
    annotate = lambda addr: L.yolo2_hip_annotate_pix(addr, 4, 4, code, dets.ctypes.data_as(C.c_void_p), 0, C.c_float(0.2), None, 0, 512, None, None)
    for shift in (1, 2, 3):
        if packedref.BPP[fmt] == 4:      # worded as YUYV's refusal
            assert L.yolo2_hip_letterbox_pix(256 + shift, 4, 4, code, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
            assert b"letterbox: a " + name + b" frame starts on a 4-byte boundary" == L.yolo2_hip_last_error()
            assert annotate(256 + shift) == hipdrv.YOLO2_ERROR
            assert b"annotate: a " + name + b" frame starts on a 4-byte boundary" == L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(256 + 2, 4, 4, 0x56595559, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"letterbox: a YUYV frame starts on a 4-byte boundary" == L.yolo2_hip_last_error()
    # what stays refused: no format has these codes, and no channel count names the new formats
    for bad in (0, 2, 7, 0x59565955, 0x3231564E ^ 0x100, code ^ 0x100, code + 1):
        assert L.yolo2_hip_letterbox_pix(256, 4, 4, bad, 512, 416, 416, None) == hipdrv.YOLO2_ERROR, hex(bad)
        err = L.yolo2_hip_last_error()
        assert b"unknown pixel format" in err and all(b"YOLO2_PIX_" + f.upper().encode() in err for f in FORMATS), err
    for ch in (4, 24, 32, 33):
        assert L.yolo2_hip_letterbox_u8(256, 4, 4, ch, 512, 416, 416, None) == hipdrv.YOLO2_ERROR, ch


# ------------------------------------------------------------------ CLI

def test_cli_help_names_the_formats():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert all(s in r.stdout for s in ("bgr24", "rgba", "bgra", "rgb0", "bgr0"))
    r = subprocess.run([CALIBRATE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stdout for s in ("bgr24", "rgba", "bgra"))


@pytest.mark.parametrize("tool", ["detect", "calibrate"])
@pytest.mark.parametrize("spelled", ["bgr24", "rgba", "bgra", "rgb0", "bgr0"])
def test_tools_parse_the_new_names(tool, spelled, tmp_path):
    """a name that parses gets as far as the missing input; nv21 and other names stop at the parser"""
    missing = str(tmp_path / "none.raw")
    argv = [CLI, "--video-raw", missing] if tool == "detect" else [CALIBRATE, "--weights", str(tmp_path / "noweights"), "--out", str(tmp_path / "o"), "--video-raw", missing]
    r = subprocess.run(argv + ["--video-pix-fmt", spelled, "--video-width", "5", "--video-height", "3"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "Unsupported --video-pix-fmt" not in r.stderr and "Unknown argument" not in r.stderr, r.stderr
    if tool == "detect":      # says what it would have read
        want = {"rgb0": "rgba", "bgr0": "bgra"}.get(spelled, spelled)
        assert f"Cannot read --video-raw {missing} (5x3 frames, --video-pix-fmt {want})" in r.stderr
    for bad in ("nv21", "rgba32", "bgr"):
        r = subprocess.run(argv + ["--video-pix-fmt", bad], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode != 0 and "Unsupported --video-pix-fmt " + bad in r.stderr
        assert "bgr24 | rgba | bgra" in r.stderr
