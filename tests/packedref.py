"""Helpers of the packed-RGB tests (tests/test_packed_host.py, tests/test_gpu_packed.py), pure numpy.  A BGR24, RGBA32 or BGRA32 frame
is by definition the RGB24 frame with the same pixels and the bytes reordered (include/yolo2_hip.h, "camera pixel formats"): byte k
(0 R, 1 G, 2 B) of pixel x is row[x * bpp + (swap ? 2 - k : k)], and a fourth byte X is never used.  to_rgb builds that RGB24 frame;
the expected side of every test is an RGB24 entry fed it."""
import numpy as np

FORMATS = ("bgr24", "rgba32", "bgra32")
BPP = {"bgr24": 3, "rgba32": 4, "bgra32": 4}
SWAP = {"bgr24": True, "rgba32": False, "bgra32": True}
# where R, G and B sit in a pixel, written out (not computed from SWAP: tests/test_packed_host.py holds the two together)
ORDER = {"bgr24": (2, 1, 0), "rgba32": (0, 1, 2), "bgra32": (2, 1, 0)}


def to_rgb(frame, fmt):
    """uint8 [h][w][3 or 4] packed frame -> the uint8 [h][w][3] RGB24 picture every entry must treat it as"""
    f = np.asarray(frame, dtype=np.uint8)
    assert f.ndim == 3 and f.shape[2] == BPP[fmt], (fmt, f.shape)
    return np.ascontiguousarray(f[..., list(ORDER[fmt])])


def from_rgb(rgb, fmt, x=None):
    """an RGB24 picture as a frame of the format.  x: the fourth byte of the 32-bit formats - a scalar or a uint8 [h][w] array (None: 0xff)"""
    p = np.asarray(rgb, dtype=np.uint8)
    assert p.ndim == 3 and p.shape[2] == 3, p.shape
    out = np.empty(p.shape[:2] + (BPP[fmt],), dtype=np.uint8)
    for k, at in enumerate(ORDER[fmt]):
        out[..., at] = p[..., k]
    if BPP[fmt] == 4:
        out[..., 3] = 0xff if x is None else x
    return out


def random_rgb(rng, w, h):
    """every byte uniform in 0..255"""
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def random_frame(rng, w, h, fmt):
    """the same picture for every format from the same generator state; the fourth byte is random too"""
    rgb = random_rgb(rng, w, h)
    x = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return from_rgb(rgb, fmt, x)
