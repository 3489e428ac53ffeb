"""The expected side of the PNG tests: numpy's restatement of the five PNG filters and of stb_image_write's selection rule (the first
filter, in order 0..4, whose sum of abs((int8_t)byte) is strictly smallest), and a reader of a PNG file's chunks."""
import struct
import zlib

import numpy as np

from jpegdec_cases import host_decode  # noqa: F401  (y2h_decode_image, pinned to stb_image by tests/test_host_codec.py)


def filtered(rgb) -> bytes:
    """uint8 [h][w][3] -> the filtered stream, a filter byte in front of every row"""
    h, w = rgb.shape[:2]
    rows = rgb.reshape(h, 3 * w).astype(np.int32)
    out = bytearray()
    for y in range(h):
        x = rows[y]
        a = np.concatenate([np.zeros(3, np.int32), x[:-3]])
        b = rows[y - 1] if y else np.zeros_like(x)
        c = np.concatenate([np.zeros(3, np.int32), b[:-3]])
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        cands = [((x - pred) & 255).astype(np.uint8) for pred in (0, a, b, (a + b) >> 1, paeth)]
        scores = [int(np.abs(cand.view(np.int8).astype(np.int32)).sum()) for cand in cands]
        t = scores.index(min(scores))
        out += bytes([t]) + cands[t].tobytes()
    return bytes(out)


def chunks(png: bytes):
    """-> [(type, data)]; the signature, every length and every CRC (against zlib.crc32) are checked, and nothing follows IEND"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        assert len(data) == n and struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data), kind
        out.append((kind, data))
        at += 12 + n
    assert at == len(png) and out[-1] == (b"IEND", b"")
    return out
