"""GPU tests of the deflate stage of the library's PNG files (csrc/kernels_png.hpp): yolo2_hip_zlib_huff against Python's
zlib.decompress at the smallest inputs at which each stage can go wrong, and byte for byte against the host writer of
libyolo2_host.so, which tests/test_png_host.py pins to zlib.  The expected side is never the code under test."""
import zlib

import numpy as np
import pytest

from yolo2_amd import hipdrv

pytestmark = pytest.mark.gpu
B, SEG = 32768, 128   # y2p::kBlock; kPngSeg, the bytes of one pack lane
C = hipdrv.C


def skewed(n, seed=0):
    """compressible bytes: geometric, so that code lengths from 1 bit to the limit occur"""
    return (np.random.default_rng(seed).geometric(0.3, n) % 256).astype(np.uint8).tobytes()


def fibonacci():
    """counts 1, 1, 2, 3, 5 ... of 19 symbols: 10945 bytes in one block whose unlimited Huffman tree is 18 deep, above the 15-bit limit"""
    f = [1, 1]
    while len(f) < 19:
        f.append(f[-1] + f[-2])
    return b"".join(bytes([7 * i]) * c for i, c in enumerate(f))


INPUTS = {f"n{n}": skewed(n, n) for n in (0, 1, SEG - 1, SEG, SEG + 1, B - 1, B, B + 1, 3 * B + 7)}
INPUTS.update({
    "single_symbol": b"\x5a" * (B + 300), "all_values_once": bytes(range(256)), "fibonacci": fibonacci(),
    "stored_between": skewed(B, 1) + np.random.default_rng(2).integers(0, 256, B, dtype=np.uint8).tobytes() + skewed(B // 2 + 5, 3),
    "one_bit_codes": (np.random.default_rng(4).random(2 * B) < 0.98).astype(np.uint8).tobytes(),
})


@pytest.mark.parametrize("name", INPUTS)
def test_zlib_huff_inflates_to_its_input_and_equals_the_host(name):
    data = INPUTS[name]
    got = hipdrv.zlib_huff(data, guard=64)
    assert zlib.decompress(got) == data
    assert got == hipdrv.zlib_huff_host(data)
    if name == "stored_between":
        assert len(got) > B + 5 and len(got) < len(data) - B // 4   # the noise block stored, the others not


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_odd_addresses_and_guard_bytes(shift):
    """the input at an odd address, the stream at another: every wide load and store has to find its own alignment"""
    data = skewed(B + 4097, shift)   # two blocks; the deflate data ends inside a second emit tile
    want = hipdrv.zlib_huff_host(data)
    cap = int(hipdrv.lib().yolo2_hip_zlib_huff_bound(len(data)))
    src = hipdrv.DevBuf(np.frombuffer(b"\0" * shift + data, dtype=np.uint8))
    dst = hipdrv.DevBuf(nbytes=cap + 64, fill=0xA5)
    size = C.c_size_t(0)
    hipdrv.check(hipdrv.lib().yolo2_hip_zlib_huff(src.addr + shift, len(data), dst.addr + 4 - shift, cap, C.byref(size)), "zlib_huff")
    out = dst.get(np.uint8, cap + 64)
    assert out[4 - shift:4 - shift + size.value].tobytes() == want
    assert (out[:4 - shift] == 0xA5).all() and (out[4 - shift + size.value:] == 0xA5).all()
    src.free()
    dst.free()


def test_refusals_come_before_any_launch():
    L = hipdrv.lib()
    buf = hipdrv.DevBuf(np.full(4096, 0xA5, dtype=np.uint8))
    size = C.c_size_t(7)
    assert L.yolo2_hip_zlib_huff_bound(100) == 100 + 6 + 6 and L.yolo2_hip_zlib_huff_bound(0) == 12
    assert L.yolo2_hip_zlib_huff(buf.addr, 100, buf.addr + 1024, 111, C.byref(size)) == hipdrv.YOLO2_ERROR
    assert b"too small" in L.yolo2_hip_last_error() and size.value == 7
    assert L.yolo2_hip_zlib_huff(0, 100, buf.addr, 4096, C.byref(size)) == hipdrv.YOLO2_ERROR
    assert L.yolo2_hip_zlib_huff(buf.addr, 100, 0, 4096, C.byref(size)) == hipdrv.YOLO2_ERROR
    assert (buf.get(np.uint8, 4096) == 0xA5).all()
    buf.free()
