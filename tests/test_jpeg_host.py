"""CPU tests of the annotated frame's JPEG stream: y2h_write_jpg_rgb24 (libyolo2_host.so), the project's statement of what the
reference's MJPEG streamer sends (stb_image_write v1.09's stbi_write_jpg_to_func with 3 components), equals the bytes the compiled
reference wrote (tests/golden/jpeg.npz), keeps to its capacity, and decodes."""
import ctypes as C
import io

import numpy as np
import pytest

import orclib
from jpegref import CASES, case, host_jpg
from yolo2_amd import hipdrv


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_byte_for_byte(name):
    rgb, quality, want = case(name)
    got = host_jpg(rgb, quality)
    assert len(got) == len(want) and got == want


def test_the_fixture_holds_the_rare_stream_ends():
    ends = {name: case(name)[2][-4:] for name in CASES}
    assert ends["seed12_15x7_q100"] == ends["seed14_4x20_q80"] == b"\xff\x00\xff\xd9"
    assert any(w % 8 and h % 8 for w, h in ((case(n)[0].shape[1], case(n)[0].shape[0]) for n in CASES))


def test_quality_is_clamped_as_the_streamer_clamps_it():
    rgb = case("rand_9x7_q80")[0]
    assert host_jpg(rgb, 0) == host_jpg(rgb, 1) == host_jpg(rgb, -7)
    assert host_jpg(rgb, 100) == host_jpg(rgb, 250)
    assert host_jpg(rgb, 1) != host_jpg(rgb, 2)


@pytest.mark.parametrize("name", CASES)
def test_bound_holds(name):
    rgb, quality, want = case(name)
    H = hipdrv.host_lib()
    assert H.y2h_jpg_rgb24_bound(rgb.shape[1], rgb.shape[0]) >= len(want)


def test_bad_sizes_are_argument_errors():
    H = hipdrv.host_lib()
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)
    out = np.zeros(4096, dtype=np.uint8)
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536)):
        assert H.y2h_write_jpg_rgb24(rgb.ctypes.data, w, h, 80, out.ctypes.data, out.size) == -1
        assert H.y2h_jpg_rgb24_bound(w, h) == 0
    assert H.y2h_write_jpg_rgb24(None, 4, 4, 80, out.ctypes.data, out.size) == -1
    assert H.y2h_jpg_rgb24_bound(65535, 65535) == 607 + 2 * ((3 * 8192 * 8192 * 1660 + 7) // 8) + 2


@pytest.mark.parametrize("name", ["rand_64x48_q80", "seed12_15x7_q100", "rand_1x1_q80"])
def test_a_small_capacity_returns_the_size_and_keeps_to_it(name):
    rgb, quality, want = case(name)
    H = hipdrv.host_lib()
    for cap in (0, 1, 606, 607, 608, len(want) - 3, len(want) - 1, len(want)):
        buf = np.full(cap + 32, 0xA5, dtype=np.uint8)
        n = H.y2h_write_jpg_rgb24(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], quality, buf.ctypes.data, cap)
        assert n == len(want), cap
        assert buf[:cap].tobytes() == want[:cap], cap
        assert (buf[cap:] == 0xA5).all(), cap


@pytest.mark.parametrize("name", CASES)
def test_the_stream_decodes(name):
    rgb, quality, _ = case(name)
    data = host_jpg(rgb, quality)
    h, w = rgb.shape[:2]
    H = orclib.host()
    H.y2h_decode_image.restype = C.c_long
    H.y2h_decode_image.argtypes = [C.c_char_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_long]
    dw, dh = C.c_int(0), C.c_int(0)
    out = np.zeros((h, w, 3), dtype=np.uint8)
    assert H.y2h_decode_image(data, len(data), C.byref(dw), C.byref(dh), out.ctypes.data, out.nbytes) == w * h * 3, H.y2h_last_error()
    assert (dw.value, dh.value) == (w, h)
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (w, h) and im.mode == "RGB"
