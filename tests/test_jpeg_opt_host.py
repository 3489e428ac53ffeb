"""CPU tests of the JPEG encoder's optimize mode on the host (y2h_write_jpg_rgb24_opt, libyolo2_host.so; csrc/jpeg_opt.hpp): the
Huffman tables are the frame's own, so what pins the mode is that the stream decodes - with the library's host decoder, which shares
nothing with the encoder - to exactly the pixels of the standard stream of the same frame and mode (the coefficients are the same:
any difference is a table or header error), and that it is never longer.  The GPU tests expect this encoder's bytes."""
import numpy as np
import pytest

from jpeg420ref import frame, host_decode
from yolo2_amd import hipdrv

enc = hipdrv.write_jpg_host
MODES = [(0, 0), (420, 0), (0, 1), (420, 4)]
FRAMES = ["1x1", "flat8x8", "crop17x9", "noise33x31", "crop48x32"]


def opt_frame(name):
    """1x1 and one colour: lone symbols, end-of-block only; 17x9: ragged MCUs; noise: many symbols, long codes; "fade" (noise whose
    amplitude halves twelve times across 640 columns, for quality 100): symbol counts over five decades - the unlimited trees of its
    AC counts are 18 (luma) and 20 (chroma) deep, so the 16-bit limit moves codes; "big" (2080x2080 noise, for quality 100): 8.4
    million chroma AC symbols, past kOptCountLimit = 2^23 - the frame that falls back."""
    if name == "1x1":
        return np.full((1, 1, 3), 200, dtype=np.uint8)
    if name == "flat8x8":
        return np.full((8, 8, 3), (10, 200, 90), dtype=np.uint8)
    if name == "fade":
        n = np.random.default_rng(640480).integers(-128, 128, (480, 640, 3)).astype(np.float64)
        return np.clip(128 + n * 2.0 ** (-12 * np.arange(640) / 640)[None, :, None], 0, 255).astype(np.uint8)
    if name == "big":
        return frame("noise", 2080, 2080)
    kind, w, h = {"crop17x9": ("crop", 17, 9), "noise33x31": ("noise", 33, 31), "crop48x32": ("crop", 48, 32)}[name]
    return frame(kind, w, h)


def dht_bits(data):
    """the four BITS lists of the stream's DHT segment, in its order (DC luma, AC luma, DC chroma, AC chroma)"""
    assert data[173:175] == b"\xff\xc4"
    at, end, out = 177, 175 + (data[175] << 8 | data[176]), []
    while at < end:
        out.append(list(data[at + 1:at + 17]))
        at += 17 + sum(out[-1])
    assert at == end and len(out) == 4
    return out


@pytest.mark.parametrize("quality", [50, 80, 100])
@pytest.mark.parametrize("subsample,restart", MODES)
@pytest.mark.parametrize("name", FRAMES)
def test_optimised_stream_decodes_to_the_standard_pixels_and_is_not_longer(name, subsample, restart, quality):
    rgb = opt_frame(name)
    std = enc(rgb, quality, subsample, restart)
    assert enc(rgb, quality, subsample, restart, optimize=False) == std
    opt = enc(rgb, quality, subsample, restart, optimize=True)
    assert len(opt) <= len(std)
    assert opt != std and np.array_equal(host_decode(opt), host_decode(std))
    # the tables list the symbols in use and no all-ones code: Kraft's sum of every table is one code short of full
    for bits in dht_bits(opt):
        assert sum(n << (16 - l) for l, n in enumerate(bits, 1)) == (1 << 16) - (1 << (16 - max(l for l, n in enumerate(bits, 1) if n)))


@pytest.mark.parametrize("subsample,restart", MODES)
def test_sixteen_bit_limit(subsample, restart):
    """quality 100 on the noise frame does not reach the limit (its AC trees are 11 and 12 deep); the fade frame does"""
    rgb = opt_frame("fade")
    std, opt = enc(rgb, 100, subsample, restart), enc(rgb, 100, subsample, restart, optimize=True)
    bits = dht_bits(opt)
    assert bits[1][15] > 0 and bits[3][15] > 0 and not any(bits[0][11:]) and not any(bits[2][11:])      # AC at 16 bits, DC within 11
    assert len(opt) < len(std) and np.array_equal(host_decode(opt), host_decode(std))


def test_fallback_frame_is_the_standard_stream():
    rgb = opt_frame("big")
    assert enc(rgb, 100, 0, 0, optimize=True) == enc(rgb, 100, 0, 0)
    assert enc(rgb[:2064, :2064], 100, 0, 0, optimize=True) != enc(rgb[:2064, :2064], 100, 0, 0)      # 8.3 million: below the limit


def test_bad_optimize_is_an_argument_error():
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)
    for optimize in (-1, 2):
        assert hipdrv.host_lib().y2h_write_jpg_rgb24_opt(rgb.ctypes.data, 4, 4, 80, 0, 0, optimize, None, 0) == -1
