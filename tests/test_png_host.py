"""CPU tests of the annotated frame as PNG, the library's own definition (csrc/png_huff.hpp): y2h_write_png_rgb24 and y2h_zlib_huff of
libyolo2_host.so against Python's zlib, zlib.crc32, the host decoder y2h_decode_image and pngref's numpy filters - never the code under
test; the stream's size beside zlib's Z_HUFFMAN_ONLY; and the surface that needs no device."""
import os
import struct
import zlib

import numpy as np
import pytest

import orclib
import pngref
from drawref import case as draw_case
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]   # 768 x 576, the decoded dog.jpg
B = 32768


def frames():
    rng = np.random.default_rng(22)
    ramp = np.add.outer(np.arange(41), np.arange(67)).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "gradient": np.stack([ramp, ramp * 2, 255 - ramp], axis=2),
            "flat": np.full((130, 90, 3), 200, dtype=np.uint8), "painted": painted(), "1x1": np.zeros((1, 1, 3), np.uint8)}


def painted():
    """the first fixture frame of the painter's golden file: boxes and labels over a picture"""
    from drawref import CASES
    return np.ascontiguousarray(draw_case(CASES[0])[4])


@pytest.mark.parametrize("name", ["noise", "gradient", "flat", "painted", "1x1"])
def test_host_png_is_valid_exact_and_filtered_by_the_rule(name):
    rgb = frames()[name]
    h, w = rgb.shape[:2]
    png = hipdrv.write_png_host(rgb)
    assert len(png) <= orclib.host().y2h_png_rgb24_bound(w, h) == 57 + 6 + h * (1 + 3 * w) + (42 * -(-h * (1 + 3 * w) // B) + 7) // 8
    (k0, ihdr), (k1, idat), _ = pngref.chunks(png)
    assert (k0, k1) == (b"IHDR", b"IDAT") and ihdr == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    assert zlib.decompress(idat) == pngref.filtered(rgb)
    assert np.array_equal(pngref.host_decode(png), rgb)


@pytest.mark.parametrize("picture", ["dog", "painted"])
def test_stream_size_beside_zlib_huffman_only(picture):
    """Allowance: zlib's Z_HUFFMAN_ONLY stream, plus what the plain header form costs at most per 32 KiB block beyond the least a
    dynamic header takes (17 + 3 * 19 + 258 * 7 bits against 17 + 3 * 4 + 258 bits: 203 bytes), plus 2 % for zlib's adaptive block
    splitting and its run-length header.  Measured: ratio 1.0013 on the dog frame, 0.9975 on the painted one
    (profiles/r22_png_rates.txt)."""
    rgb = DOG if picture == "dog" else painted()
    filt = pngref.filtered(rgb)
    ours = len(hipdrv.zlib_huff_host(filt))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    theirs = len(co.compress(filt) + co.flush())
    blocks = -(-len(filt) // B)
    print(f"{picture}: {ours} bytes, zlib Z_HUFFMAN_ONLY {theirs}, ratio {ours / theirs:.4f}, level 6 {len(zlib.compress(filt, 6))}")
    assert ours <= theirs * 1.02 + 203 * blocks, f"ratio {ours / theirs:.4f}"
    assert ours / theirs <= 1.05, f"ratio {ours / theirs:.4f}"


def test_surface_without_a_device():
    header = open(os.path.join(ROOT, "include", "yolo2_hip.h")).read()
    for name in ("yolo2_hip_zlib_huff_bound", "yolo2_hip_zlib_huff"):
        assert name in hipdrv.EXPORTS and name + "(" in header
    assert "annotated frames as PNG" in header and "NO LZ matches" in header
    assert "png" in open(os.path.join(ROOT, "README.md")).read().lower()
    H = orclib.host()
    assert hipdrv.host_lib().y2h_png_rgb24_bound(0, 4) == 0 and hipdrv.host_lib().y2h_png_rgb24_bound(65536, 1) == 0
    assert H.y2h_write_png_rgb24(None, 4, 4, None, 0) == -1 and b"write_png_rgb24" in H.y2h_last_error()
    with pytest.raises(ValueError):
        hipdrv.write_png_host(np.zeros((4, 4), np.uint8))
