"""What tests/test_jpeg420_host.py and tests/test_gpu_jpeg420.py share: the frames (seeded noise and crops of the dog frame), the MCU
geometry of a mode, and y2h_decode_image, the host decoder that tests/test_host_codec.py pins to the reference's stb_image."""
import ctypes as C
import os

import numpy as np

import orclib

DOG = np.load(os.path.join(orclib.ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
SHAPES = [(1, 1), (16, 16), (17, 15), (48, 48), (320, 240)]


def frame(kind, w, h):
    """"noise": every byte random (long codes, 0xFF bytes, large DC differences); "crop": the dog frame from (200, 100)"""
    if kind == "noise":
        return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.ascontiguousarray(DOG[100:100 + h, 200:200 + w])


def mcus(w, h, subsample):
    """-> MCUs per row, MCUs"""
    m = 16 if subsample == 420 else 8
    return -(-w // m), -(-w // m) * -(-h // m)


def restarts(w, h, subsample):
    """the intervals every shape runs with: none, one MCU, an MCU row, 7 (divides little), at least the whole scan"""
    per_row, n = mcus(w, h, subsample)
    return [0, 1, per_row, 7, n + 3]


def host_decode(data):
    """y2h_decode_image -> uint8 [h][w][3]"""
    H = orclib.host()
    H.y2h_decode_image.restype = C.c_long
    H.y2h_decode_image.argtypes = [C.c_char_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_long]
    w, h = C.c_int(0), C.c_int(0)
    assert H.y2h_decode_image(data, len(data), C.byref(w), C.byref(h), None, 0) == -2, H.y2h_last_error()   # (-2: the size is known, no room)
    out = np.zeros((h.value, w.value, 3), dtype=np.uint8)
    assert H.y2h_decode_image(data, len(data), C.byref(w), C.byref(h), out.ctypes.data, out.nbytes) == out.nbytes, H.y2h_last_error()
    return out
