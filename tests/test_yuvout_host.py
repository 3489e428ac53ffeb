"""CPU tests of the loop's YUV 4:2:0 output (YOLO2_LOOP_OUT_NV12 / _I420): y2h_rgb24_to_yuv420 (libyolo2_host.so), the host restatement of
what the 4:2:0 painters compute, against literal colours worked out by hand and against the numpy side yuvoutref.from_rgb; the round
trip through y2h_yuv420_to_rgb24; and the refusals that need no device - the host function's, hipdrv's, the CLI's - with the header and
INTEGRATION.md."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import orclib
import yuv420ref
import yuvoutref
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
HEADER = os.path.join(ROOT, "include", "yolo2_hip.h")
FORMATS = ("nv12", "i420")
# (R, G, B) -> (Y, U, V) of a flat block, by hand from the formula of include/yolo2_hip.h
COLOURS = {"white": ((255, 255, 255), (235, 128, 128)), "black": ((0, 0, 0), (16, 128, 128)), "red": ((255, 0, 0), (82, 90, 240)),
           "green": ((0, 255, 0), (144, 54, 34)), "blue": ((0, 0, 255), (41, 240, 110))}
SIZES = ((2, 2), (4, 2), (2, 4), (6, 2), (6, 6), (34, 18))


def host():
    lib = orclib.host()
    lib.y2h_rgb24_to_yuv420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.y2h_rgb24_to_yuv420.restype = C.c_int
    lib.y2h_yuv420_to_rgb24.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.y2h_yuv420_to_rgb24.restype = C.c_int
    return lib


def to_yuv(rgb, fmt):
    """y2h_rgb24_to_yuv420 on uint8 [h][w][3] -> uint8 [h * 3 / 2][w], with 8 guard bytes behind the frame checked"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    out = np.full(w * h * 3 // 2 + 8, 0xA5, dtype=np.uint8)
    assert host().y2h_rgb24_to_yuv420(rgb.ctypes.data, w, h, int(fmt == "nv12"), out.ctypes.data) == 0
    assert (out[-8:] == 0xA5).all()
    return out[:-8].reshape(h * 3 // 2, w)


@pytest.mark.parametrize("fmt", FORMATS)
def test_literal_colours_on_2x2_frames(fmt):
    """a 2 x 2 frame is Y Y Y Y U V in both layouts"""
    for name, (rgb, yuv) in COLOURS.items():
        got = to_yuv(np.full((2, 2, 3), rgb, dtype=np.uint8), fmt)
        assert got.reshape(-1).tolist() == [yuv[0]] * 4 + [yuv[1], yuv[2]], name


@pytest.mark.parametrize("fmt", FORMATS)
def test_chroma_is_taken_from_the_blocks_mean_colour(fmt):
    """{red, green, blue, white}: the block's sum is grey, so U = V = 128, which no single one of its pixels has"""
    block = np.array([[COLOURS["red"][0], COLOURS["green"][0]], [COLOURS["blue"][0], COLOURS["white"][0]]], dtype=np.uint8)
    assert to_yuv(block, fmt).reshape(-1).tolist() == [82, 144, 41, 235, 128, 128]
    assert all(COLOURS[c][1][1:] != (128, 128) for c in ("red", "green", "blue"))


def test_layouts_by_hand():
    """4 x 2, two blocks red | green.  NV12: U V U V; I420: U U, then V V"""
    rgb = np.zeros((2, 4, 3), dtype=np.uint8)
    rgb[:, :2] = COLOURS["red"][0]
    rgb[:, 2:] = COLOURS["green"][0]
    assert to_yuv(rgb, "nv12").reshape(-1).tolist() == [82, 82, 144, 144] * 2 + [90, 240, 54, 34]
    assert to_yuv(rgb, "i420").reshape(-1).tolist() == [82, 82, 144, 144] * 2 + [90, 54, 240, 34]
    rgb = np.zeros((4, 2, 3), dtype=np.uint8)      # 2 x 4, red over green: chroma rows U V / U V, or the U column then the V column
    rgb[:2] = COLOURS["red"][0]
    rgb[2:] = COLOURS["green"][0]
    assert to_yuv(rgb, "nv12").reshape(-1).tolist() == [82] * 4 + [144] * 4 + [90, 240, 54, 34]
    assert to_yuv(rgb, "i420").reshape(-1).tolist() == [82] * 4 + [144] * 4 + [90, 54, 240, 34]
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)      # 4 x 4, quadrants red blue / green white
    rgb[:2, :2], rgb[:2, 2:], rgb[2:, :2], rgb[2:, 2:] = (COLOURS[c][0] for c in ("red", "blue", "green", "white"))
    ys = [82, 82, 41, 41] * 2 + [144, 144, 235, 235] * 2
    assert to_yuv(rgb, "nv12").reshape(-1).tolist() == ys + [90, 240, 240, 110, 54, 34, 128, 128]
    assert to_yuv(rgb, "i420").reshape(-1).tolist() == ys + [90, 240, 54, 128] + [240, 110, 34, 128]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", SIZES)
def test_host_function_equals_the_numpy_side_on_random_frames(fmt, w, h):
    rgb = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert np.array_equal(to_yuv(rgb, fmt), yuvoutref.from_rgb(rgb, fmt))
    assert np.array_equal(hipdrv.rgb24_to_yuv420(rgb, fmt), yuvoutref.from_rgb(rgb, fmt))


def test_every_colour_as_a_flat_block_and_the_round_trip():
    """256 frames of 512 x 512: frame R holds colour (R, G, B) as the flat 2 x 2 block (G, B).  The first frames are compared element
    by element, all of them by the sha256 of both sides; each comes back through y2h_yuv420_to_rgb24 within (2, 2, 3) levels of
    R, G, B - the bound of the forward / inverse pair on flat blocks (include/yolo2_hip.h)."""
    lib = host()
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgb = np.empty((512, 512, 3), dtype=np.uint8)
    rgb[..., 1] = np.repeat(np.repeat(g, 2, axis=0), 2, axis=1)
    rgb[..., 2] = np.repeat(np.repeat(b, 2, axis=0), 2, axis=1)
    back = np.empty_like(rgb)
    worst = np.zeros(3, dtype=np.int64)
    for r in range(256):
        rgb[..., 0] = r
        want = yuvoutref.from_rgb(rgb, "nv12")
        y, u, v = yuv420ref.planes(want, "nv12")
        for fmt in FORMATS:
            expect = want if fmt == "nv12" else yuv420ref.pack(y, u, v, "i420")
            got = to_yuv(rgb, fmt)
            if r < 4 or r == 255:
                assert np.array_equal(got, expect), (r, fmt)
            assert hashlib.sha256(got.tobytes()).digest() == hashlib.sha256(expect.tobytes()).digest(), (r, fmt)
            if fmt == "nv12":      # (the I420 frame holds the same planes: the hashes above say so)
                assert lib.y2h_yuv420_to_rgb24(got.ctypes.data, back.ctypes.data, 512, 512, 1) == 0
                worst = np.maximum(worst, np.abs(back.astype(np.int16) - rgb.astype(np.int16)).reshape(-1, 3).max(axis=0))
    print("round trip, worst |difference| of R, G, B over all colours:", worst.tolist())
    assert worst[0] <= 2 and worst[1] <= 2 and worst[2] <= 3


def test_host_function_refuses_null_and_bad_sizes_with_the_output_untouched():
    lib = host()
    rgb = np.zeros(64, dtype=np.uint8)
    out = np.full(64, 0xA5, dtype=np.uint8)
    for w, h in ((0, 2), (3, 2), (2, 3), (-2, 2)):
        for semi in (0, 1):
            assert lib.y2h_rgb24_to_yuv420(rgb.ctypes.data, w, h, semi, out.ctypes.data) != 0, (w, h)
            assert f"{w}x{h}".encode() in lib.y2h_last_error()
    assert lib.y2h_rgb24_to_yuv420(None, 2, 2, 1, out.ctypes.data) != 0
    assert lib.y2h_rgb24_to_yuv420(rgb.ctypes.data, 2, 2, 0, None) != 0
    assert (out == 0xA5).all()
    with pytest.raises(ValueError, match="3x2"):
        hipdrv.rgb24_to_yuv420(np.zeros((2, 3, 3), dtype=np.uint8), "nv12")
    with pytest.raises(ValueError, match="fmt"):
        hipdrv.rgb24_to_yuv420(np.zeros((2, 2, 3), dtype=np.uint8), "nv21")


def test_python_checks_out_order_before_any_call():
    frame = np.zeros((4, 4, 3), dtype=np.uint8)
    for call in (hipdrv.loop_images, hipdrv.loop_jpegs):
        for fmt in FORMATS:
            with pytest.raises(ValueError, match="jpeg_quality"):
                call(None, [frame], jpeg_quality=80, out_order=fmt)
        with pytest.raises(ValueError, match="out_order"):
            call(None, [frame], out_order="nv21")
    assert hipdrv.LOOP_OUT_NV12 == hipdrv.pix_code("nv12") == 0x3231564E and hipdrv.LOOP_OUT_I420 == hipdrv.pix_code("i420") == 0x32315559
    assert hipdrv._loop_out_format("nv12", None) == hipdrv.LOOP_OUT_NV12 and hipdrv._loop_out_format("i420", None) == hipdrv.LOOP_OUT_I420
    assert hipdrv._loop_out_format("rgb", None) == 0 and hipdrv._loop_out_format("rgb", 80) == 1


def test_library_refuses_odd_sizes_and_short_buffers_without_a_device():
    """y2_loop_check runs before the context is looked at: a handle that is never dereferenced serves"""
    L = hipdrv.lib()
    dummy = C.c_void_p(1 << 20)
    kw = dict(precision=0, flags=hipdrv.DETS_BEST_CLASS, thresh=0.2, nms=0.45, batch=2, cap=8, labels=None, quality=0)

    def raw(sizes, out_format, caps):
        frames = [np.zeros((h, w, 3), dtype=np.uint8) for w, h in sizes]
        r = hipdrv.loop_images_raw(dummy, frames, "rgb24", kw["precision"], kw["flags"], kw["thresh"], kw["nms"], kw["batch"], kw["cap"], None,
                                   out_format, 0, caps, guard=8)
        assert r[0] == hipdrv.YOLO2_ERROR and all((o == 0xA5).all() for o in r[4]) and not r[2].any() and not r[5].any()
        return L.yolo2_hip_last_error()
    for code in (hipdrv.LOOP_OUT_NV12, hipdrv.LOOP_OUT_I420):
        err = raw([(4, 4), (5, 4)], code, [24, 30])
        assert b"frame 1" in err and b"5x4" in err and b"odd" in err, err
        err = raw([(4, 5), (4, 4)], code, [30, 24])
        assert b"frame 0" in err and b"4x5" in err and b"odd" in err, err
        err = raw([(4, 4), (6, 4)], code, [24, 35])
        assert b"output buffer too small for frame 1 (35 < 36 bytes)" in err, err
    assert b"unknown output format 2 " in raw([(4, 4)], 2, [48])
    assert b"unknown output format" in raw([(4, 4)], hipdrv.LOOP_OUT_NV12 ^ 0x100, [48])


def _cli(args, cwd):
    return subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                           os.path.join(PKG, "config", "coco.names")] + args, capture_output=True, text=True, cwd=str(cwd),
                          env=dict(os.environ, YOLO2_NO_DUMP="1"))


@pytest.mark.parametrize("spelled", ["nv12", "yuv420p", "i420"])
def test_cli_takes_the_formats_with_the_loop_only(spelled, tmp_path):
    (tmp_path / "video.rgb").write_bytes(bytes(8 * 6 * 3 * 2))
    base = ["--weights", str(tmp_path / "none"), "--video-raw", str(tmp_path / "video.rgb"), "--video-width", "8", "--video-height", "6", "--post", "gpu",
            "--annotate-gpu", "--save-annotated-dir", str(tmp_path / "d"), "--annotated-format", spelled]
    r = _cli(base, tmp_path)
    want = "yuv420p" if spelled == "i420" else spelled
    assert r.returncode != 0 and f"--annotated-format {want} needs --loop-gpu" in r.stderr, r.stderr
    # with the loop the argument checks pass: the run fails later, for its missing weights (without a GPU: for the missing device)
    r = _cli(base + ["--loop-gpu"], tmp_path)
    assert r.returncode != 0 and "--annotated-format" not in r.stderr and "--loop-gpu" not in r.stderr, r.stderr
    assert "streaming (" in r.stdout and r.stderr.startswith("Fatal error: ")
    r = _cli(base[:-1] + ["nv21", "--loop-gpu"], tmp_path)
    assert r.returncode != 0 and "--annotated-format is ppm, jpg, nv12 or yuv420p, not nv21" in r.stderr
    r = subprocess.run([os.path.join(PKG, "yolov2_detect"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "nv12 | yuv420p" in r.stdout and "frame_NNNNNN.nv12" in r.stdout and "frame_NNNNNN.yuv" in r.stdout


def test_header_python_and_integration_guide_name_the_formats():
    text = open(HEADER).read()
    code = " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split())
    assert "YOLO2_LOOP_OUT_NV12 = 0x3231564E" in code and "YOLO2_LOOP_OUT_I420 = 0x32315559" in code
    doc = " ".join(text.replace("\n *", " ").split())
    for phrase in ("y2h_rgb24_to_yuv420", "Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16", "(-38 Rs - 74 Gs + 112 Bs + 512) >> 10",
                   "(112 Rs - 94 Gs - 18 Bs + 512) >> 10", "identity with swscale's YUV is not claimed", "the reference has no YUV output"):
        assert phrase in doc, phrase
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_index.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr or r.stdout
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "YOLO2_LOOP_OUT_NV12" in guide and "YOLO2_LOOP_OUT_I420" in guide and "y2h_rgb24_to_yuv420" in guide
    for cls in (hipdrv.Yolo2Hip, hipdrv.Yolo2HipMulti):
        assert callable(cls.loop_images) and callable(cls.loop_jpegs)
