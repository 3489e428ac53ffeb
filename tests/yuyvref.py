"""Helpers of the YUYV tests (tests/test_yuyv_host.py, tests/test_gpu_yuyv.py): the issue's arithmetic in numpy, which the CPU tests
pin to the frames and the exhaustive sha256 the compiled reference produced (tests/golden/yuyv.npz), and a way to make natural YUYV
inputs from an RGB image."""
import numpy as np


def formula(yuyv):
    """uint8 [h][w][2] packed YUYV 4:2:2 -> uint8 [h][w][3]: c = Y - 16, d = U - 128, e = V - 128, (.. + 128) >> 8 with an arithmetic
    shift (numpy's >> on signed integers floors), clamped to 0..255 (linux_app/src/yolo2_v4l2.c:328-374)"""
    f = np.ascontiguousarray(yuyv, dtype=np.uint8).astype(np.int64)
    c = f[..., 0] - 16
    d = np.repeat(f[:, 0::2, 1], 2, axis=1) - 128
    e = np.repeat(f[:, 1::2, 1], 2, axis=1) - 128
    rgb = np.stack([(298 * c + 409 * e + 128) >> 8, (298 * c - 100 * d - 208 * e + 128) >> 8, (298 * c + 516 * d + 128) >> 8], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def rgb_to_yuyv(rgb):
    """a natural YUYV frame from an RGB image of even width (BT.601 studio range, chroma of the pair's mean).  Only ever an INPUT."""
    p = np.asarray(rgb, dtype=np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 16 + (65.738 * r + 129.057 * g + 25.064 * b) / 256
    u = 128 + (-37.945 * r - 74.494 * g + 112.439 * b) / 256
    v = 128 + (112.439 * r - 94.154 * g - 18.285 * b) / 256
    out = np.empty(y.shape + (2,), dtype=np.uint8)
    out[..., 0] = np.clip(np.rint(y), 0, 255)
    out[:, 0::2, 1] = np.clip(np.rint((u[:, 0::2] + u[:, 1::2]) / 2), 0, 255)
    out[:, 1::2, 1] = np.clip(np.rint((v[:, 0::2] + v[:, 1::2]) / 2), 0, 255)
    return out


def exhaustive_frame(y):
    """512 x 256 frame whose pairs are (y, u, 255 - y, v), u = row, v = pair within the row: y = 0..255 gives every (Y, U, V) triple"""
    f = np.empty((256, 256, 4), dtype=np.uint8)
    f[:, :, 0] = y
    f[:, :, 1] = np.arange(256, dtype=np.uint8)[:, None]
    f[:, :, 2] = 255 - y
    f[:, :, 3] = np.arange(256, dtype=np.uint8)[None, :]
    return f.reshape(256, 512, 2)
