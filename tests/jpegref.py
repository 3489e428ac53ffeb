"""Helpers of the JPEG tests (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py): the cases of tests/golden/jpeg.npz - frames, qualities
and the bytes the compiled reference's stbi_write_jpg_to_func wrote for them (tests/golden/make_jpeg_golden.py) - and
y2h_write_jpg_rgb24 (libyolo2_host.so), the host restatement the CPU tests pin to them and the GPU tests expect at other sizes."""
import os

import numpy as np

import orclib
from yolo2_amd import hipdrv

GOLD = np.load(os.path.join(orclib.ROOT, "tests", "golden", "jpeg.npz"))
CASES = [str(c) for c in GOLD["names"]]


def case(name):
    """-> frame uint8 [h][w][3], quality, the reference's stream (bytes)"""
    return GOLD[name + "/rgb"], int(GOLD[name + "/quality"]), GOLD[name + "/jpg"].tobytes()


def host_jpg(rgb, quality):
    """y2h_write_jpg_rgb24 -> bytes"""
    return hipdrv.write_jpg_host(rgb, quality)
