"""Helpers of the planar YUV 4:2:0 tests (tests/test_yuv420_host.py, tests/test_gpu_yuv420.py), pure numpy.  An NV12 or I420 frame is
by definition the YUYV frame whose row y is Y0 U Y1 V from luma row y and chroma row y >> 1 (include/yolo2_hip.h, "camera pixel
formats"): to_yuyv builds that frame, and the expected side of every test is yuyvref.formula(to_yuyv(frame)) - the arithmetic
tests/test_yuyv_host.py pins to the compiled reference - through an RGB24 entry."""
import numpy as np

import yuyvref

FORMATS = ("nv12", "i420")


def planes(frame, fmt):
    """uint8 [h * 3 / 2][w] -> (Y [h][w], U [h/2][w/2], V [h/2][w/2]) views of the frame's bytes"""
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    assert f.ndim == 2 and f.shape[0] % 3 == 0 and f.shape[1] % 2 == 0, f.shape
    w, h = f.shape[1], f.shape[0] * 2 // 3
    flat = f.reshape(-1)
    y, c = flat[:w * h].reshape(h, w), flat[w * h:]
    if fmt == "nv12":
        uv = c.reshape(h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    assert fmt == "i420", fmt
    q = (w // 2) * (h // 2)
    return y, c[:q].reshape(h // 2, w // 2), c[q:].reshape(h // 2, w // 2)


def to_yuyv(frame, fmt):
    """uint8 [h * 3 / 2][w] NV12 / I420 frame -> the uint8 [h][w][2] YUYV frame it stands for: chroma replicated down the two rows of a block"""
    y, u, v = planes(frame, fmt)
    out = np.empty(y.shape + (2,), dtype=np.uint8)
    out[..., 0] = y
    out[:, 0::2, 1] = np.repeat(u, 2, axis=0)
    out[:, 1::2, 1] = np.repeat(v, 2, axis=0)
    return out


def to_rgb(frame, fmt):
    """the RGB24 picture every entry must treat the frame as"""
    return yuyvref.formula(to_yuyv(frame, fmt))


def pack(y, u, v, fmt):
    """planes -> uint8 [h * 3 / 2][w]"""
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and u.shape == v.shape == (h // 2, w // 2)
    chroma = np.stack([u, v], axis=-1).reshape(-1) if fmt == "nv12" else np.concatenate([u.reshape(-1), v.reshape(-1)])
    assert fmt in FORMATS, fmt
    return np.concatenate([np.asarray(y, dtype=np.uint8).reshape(-1), chroma.astype(np.uint8)]).reshape(h * 3 // 2, w)


def random_frame(rng, w, h, fmt):
    """every byte uniform in 0..255 (both clamps are hit); the same picture for both formats from the same generator state"""
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    return pack(y, u, v, fmt)


def from_rgb(rgb, fmt):
    """a natural frame from an RGB image of even width and height (BT.601 studio range, chroma of the block's mean).  Only ever an INPUT."""
    p = np.asarray(rgb, dtype=np.float64)
    h, w = p.shape[:2]
    assert h % 2 == 0 and w % 2 == 0, p.shape
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 16 + (65.738 * r + 129.057 * g + 25.064 * b) / 256
    u = 128 + (-37.945 * r - 74.494 * g + 112.439 * b) / 256
    v = 128 + (112.439 * r - 94.154 * g - 18.285 * b) / 256
    mean = lambda a: a.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return pack(q(y), q(mean(u)), q(mean(v)), fmt)


def exhaustive_frame(y, fmt):
    """like yuyvref.exhaustive_frame: a 512 x 512 frame whose luma is y on even and 255 - y on odd columns and whose chroma block (i, j)
    is (U, V) = (i, j).  A chroma pair is shared by four pixels, two of each luma, so y = 0..255 still gives every (Y, U, V) triple."""
    luma = np.empty((512, 512), dtype=np.uint8)
    luma[:, 0::2] = y
    luma[:, 1::2] = 255 - y
    u = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None], (256, 256))
    v = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :], (256, 256))
    return pack(luma, u, v, fmt)
