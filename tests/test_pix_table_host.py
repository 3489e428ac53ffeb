"""CPU tests of the one pixel-format list (csrc/pix_formats.hpp) as its users show it: hipdrv's names against the public YOLO2_PIX_*
constants, the library's descriptor rules through yolo2_hip_letterbox_pix (dummy non-null addresses: every case is refused before any
launch, so no GPU is needed), and --video-pix-fmt of both CLIs on the paths that end before anything is loaded.  The expected
messages are written out: they are what the library and the CLIs printed before the list existed.
yolov2_calibrate has no "cannot read" path of its own before the GPU is opened; its parser is checked by what follows the option: an
accepted spelling reaches the next argument (a made-up one, refused as unknown), an unsupported one is refused first."""
import os
import re
import subprocess

import pytest

import orclib
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
HEADER = os.path.join(ROOT, "include", "yolo2_hip.h")

NAMES = {**hipdrv.PIXFMTS, **hipdrv.PIXFMTS_420, **hipdrv.PIXFMTS_PACKED, **hipdrv.PIXFMTS_BAYER}
# the library's name of each format, and its rules (include/yolo2_hip.h's table of the formats)
LIB_NAME = {"grey8": "GREY8", "rgb24": "RGB24", "yuyv": "YUYV", "nv12": "NV12", "i420": "I420", "bgr24": "BGR24", "rgba32": "RGBA32", "bgra32": "BGRA32",
            "bayer_rggb8": "BAYER_RGGB8", "bayer_bggr8": "BAYER_BGGR8", "bayer_grbg8": "BAYER_GRBG8", "bayer_gbrg8": "BAYER_GBRG8"}
EVEN_W, EVEN_H, ALIGN4 = ("yuyv", "nv12", "i420"), ("nv12", "i420"), ("yuyv", "rgba32", "bgra32")
BAYER = ("bayer_rggb8", "bayer_bggr8", "bayer_grbg8", "bayer_gbrg8")
UNKNOWN = ("unknown pixel format 0x2 (YOLO2_PIX_GREY8, YOLO2_PIX_RGB24, YOLO2_PIX_YUYV, YOLO2_PIX_NV12, YOLO2_PIX_I420, YOLO2_PIX_BGR24, "
           "YOLO2_PIX_RGBA32 or YOLO2_PIX_BGRA32; YOLO2_PIX_BAYER_RGGB8, _BGGR8, _GRBG8 or _GBRG8)")
# --video-pix-fmt: every spelling and the canonical one it stands for
SPELLINGS = {"rgb24": "rgb24", "yuyv422": "yuyv422", "yuyv": "yuyv422", "nv12": "nv12", "yuv420p": "yuv420p", "i420": "yuv420p", "bgr24": "bgr24",
             "rgba": "rgba", "rgb0": "rgba", "bgra": "bgra", "bgr0": "bgra", "bayer_rggb8": "bayer_rggb8", "bayer_bggr8": "bayer_bggr8",
             "bayer_grbg8": "bayer_grbg8", "bayer_gbrg8": "bayer_gbrg8"}
UNSUPPORTED = ("Unsupported --video-pix-fmt %s (rgb24 | yuyv422 | nv12 | yuv420p | bgr24 | rgba | bgra | bayer_rggb8 | bayer_bggr8 | bayer_grbg8 | "
               "bayer_gbrg8)")


def test_every_public_constant_has_exactly_one_hipdrv_name():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    consts = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"\b(YOLO2_PIX_\w+)\s*=\s*(0x[0-9A-Fa-f]+|\d+)", text)}
    assert len(consts) == 12 and len(NAMES) == 12
    assert len(hipdrv.PIXFMTS) + len(hipdrv.PIXFMTS_420) + len(hipdrv.PIXFMTS_PACKED) + len(hipdrv.PIXFMTS_BAYER) == 12   # no name in two tables
    for const, value in consts.items():
        assert [n for n, v in NAMES.items() if v == value] == [const[len("YOLO2_PIX_"):].lower()], const
    assert sorted(NAMES.values()) == sorted(consts.values())      # no hipdrv name without a constant
    for name, value in NAMES.items():
        assert hipdrv.pix_code(name) == value
    assert set(LIB_NAME) == set(NAMES)


def _refused(name, addr, w, h):
    L = hipdrv.lib()
    assert L.yolo2_hip_letterbox_pix(addr, w, h, NAMES[name], 512, 416, 416, None) == hipdrv.YOLO2_ERROR, (name, addr, w, h)
    return L.yolo2_hip_last_error().decode()


@pytest.mark.parametrize("name", sorted(LIB_NAME))
def test_descriptor_rules_through_letterbox_pix(name):
    """the cases a format's descriptor refuses; a case it allows would launch, so it is not tried here (tests/test_gpu_*.py run those)"""
    lib_name = LIB_NAME[name]
    if name in EVEN_W:
        assert _refused(name, 256, 5, 4) == f"letterbox: {lib_name} frames have an even width, not 5"
    if name in EVEN_H:
        assert _refused(name, 256, 4, 5) == f"letterbox: {lib_name} frames have an even height, not 5"
    if name in BAYER:
        assert _refused(name, 256, 1, 1) == f"letterbox: {lib_name} frames are at least 2x2, not 1x1"
    if name in ALIGN4:
        assert _refused(name, 257, 4, 4) == f"letterbox: a {lib_name} frame starts on a 4-byte boundary"
    assert _refused(name, 0, 4, 4) == "null buffer address"      # every format, whatever its rules


def test_unknown_fourcc_message():
    L = hipdrv.lib()
    assert L.yolo2_hip_letterbox_pix(256, 4, 4, 2, 512, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert L.yolo2_hip_last_error().decode() == UNKNOWN


def _stderr_line(argv, cwd):
    r = subprocess.run(argv, capture_output=True, text=True, cwd=str(cwd))
    assert r.returncode == 1, (argv, r.stderr)
    return r.stderr.split("\n")[0]


@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_detect_accepts_every_spelling_and_reports_the_canonical_one(spelling, tmp_path):
    raw = str(tmp_path / "none.raw")
    line = _stderr_line([os.path.join(PKG, "yolov2_detect"), "--video-raw", raw, "--video-width", "64", "--video-height", "48", "--video-pix-fmt", spelling],
                        tmp_path)
    assert line == f"Cannot read --video-raw {raw} (64x48 frames, --video-pix-fmt {SPELLINGS[spelling]})"


@pytest.mark.parametrize("cli", ["yolov2_detect", "yolov2_calibrate"])
@pytest.mark.parametrize("spelling", ["uyvy", "grey8", "RGB24", ""])
def test_clis_refuse_an_unsupported_spelling(cli, spelling, tmp_path):
    line = _stderr_line([os.path.join(PKG, cli), "--video-raw", str(tmp_path / "none.raw"), "--video-pix-fmt", spelling, "--no-such-option"], tmp_path)
    assert line == UNSUPPORTED % spelling


@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_calibrate_accepts_every_spelling(spelling, tmp_path):
    line = _stderr_line([os.path.join(PKG, "yolov2_calibrate"), "--video-raw", str(tmp_path / "none.raw"), "--video-pix-fmt", spelling, "--no-such-option"],
                        tmp_path)
    assert line == "Unknown argument: --no-such-option"
