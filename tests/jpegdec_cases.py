"""What tests/test_jpegdec_host.py and tests/test_gpu_jpegdec.py share: the JPEG fixtures of tests/golden/images.npz, the host decoder
(y2h_decode_image, pinned to stb_image by tests/test_host_codec.py) as the expected side, a header reader of its own for the expected
classification, and the damaged copies of three streams."""
import ctypes
import functools
import os

import numpy as np

import orclib

IMAGES = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images.npz"))
JPEGS = [str(n) for n in IMAGES["names"] if f"{n}/file" in IMAGES and IMAGES[f"{n}/file"][:2].tobytes() == b"\xff\xd8"]


def stream(name: str) -> bytes:
    return IMAGES[f"{name}/file"].tobytes()


def host_decode(data: bytes):
    """y2h_decode_image -> uint8 [h][w][3], or None where the host decoder throws"""
    H = orclib.host()
    H.y2h_decode_image.restype = ctypes.c_long
    H.y2h_decode_image.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    buf = np.zeros(1400 * 1000 * 3, dtype=np.uint8)
    n = H.y2h_decode_image(data, len(data), ctypes.byref(w), ctypes.byref(h), buf.ctypes.data_as(ctypes.c_void_p), buf.size)
    return None if n < 0 else buf[:n].reshape(h.value, w.value, 3).copy()


@functools.lru_cache(maxsize=None)
def host_decode_fixture(name: str):
    out = host_decode(stream(name))
    out.setflags(write=False)
    return out


def write_jpg(rgb: np.ndarray, quality: int) -> bytes:
    """y2h_write_jpg_rgb24: baseline, 4:4:4, no DRI, the Annex K tables scaled by `quality`"""
    from yolo2_amd import hipdrv
    return hipdrv.write_jpg_host(np.ascontiguousarray(rgb, dtype=np.uint8), quality)


def header_facts(data: bytes) -> dict:
    """SOF type, size, component count, DRI and the offset of the entropy-coded data, read segment by segment"""
    assert data[:2] == b"\xff\xd8"
    i, facts = 2, {"dri": 0}
    while i + 4 <= len(data):
        assert data[i] == 0xFF, i
        m, L = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            facts.update(sof=m, height=(data[i + 5] << 8) | data[i + 6], width=(data[i + 7] << 8) | data[i + 8], ncomp=data[i + 9])
        if m == 0xDD:
            facts["dri"] = (data[i + 4] << 8) | data[i + 5]
        if m == 0xDA:
            facts["scan"] = i + 2 + L
            return facts
        i += 2 + L
    raise AssertionError("no SOS")


def rst_positions(data: bytes, scan: int):
    return [i for i in range(scan, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


DAMAGE_SOURCES = ("jpg/base_420", "jpg/restart_blocks", "jpg/restart_rows")


@functools.lru_cache(maxsize=None)
def damaged():
    """{label: bytes}: truncated mid-scan, an RST marker removed / duplicated (the streams that have some), a byte overwritten
    inside the scan, a stray FFD9 mid-scan"""
    out = {}
    for src in DAMAGE_SOURCES:
        d = stream(src)
        scan = header_facts(d)["scan"]
        mid = scan + (len(d) - scan) // 2
        out[f"{src}:truncated"] = d[:mid]
        rst = rst_positions(d, scan)
        if rst:
            r = rst[len(rst) // 2]
            out[f"{src}:rst_removed"] = d[:r] + d[r + 2:]
            out[f"{src}:rst_duplicated"] = d[:r] + d[r:r + 2] + d[r:]
        for k, at in enumerate((scan + 5, mid, len(d) - 6)):
            b = bytearray(d)
            b[at] ^= 0x5A
            out[f"{src}:byte{k}"] = bytes(b)
        out[f"{src}:stray_eoi"] = d[:mid] + b"\xff\xd9" + d[mid:]
    return out
