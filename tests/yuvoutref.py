"""The loop's YUV 4:2:0 OUTPUT (YOLO2_LOOP_OUT_NV12 / _I420, include/yolo2_hip.h) as pure numpy: the definition restated, in int64 with
floor shifts.  from_rgb(rgb, fmt) is the expected side of tests/test_yuvout_host.py and tests/test_gpu_yuvout.py, applied to RGB24
results of the same build (which the loop's own tests pin).  It is never the code under test.

    per pixel      Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
    per 2x2 block  U = ((-38 Rs - 74 Gs + 112 Bs + 512) >> 10) + 128,  V = ((112 Rs - 94 Gs - 18 Bs + 512) >> 10) + 128

with Rs, Gs, Bs the sums over the block's four pixels.  No clamp: Y lies in 16..235, U and V in 16..240 for every colour."""
import numpy as np

import yuv420ref

FORMATS = yuv420ref.FORMATS


def from_rgb(rgb, fmt):
    """uint8 [h][w][3] (w, h even) -> uint8 [h * 3 / 2][w]: Y [h][w], then NV12's U V rows [h/2][w] or I420's U and V planes"""
    p = np.asarray(rgb)
    assert p.dtype == np.uint8 and p.ndim == 3 and p.shape[2] == 3 and p.shape[0] % 2 == 0 and p.shape[1] % 2 == 0, (p.dtype, p.shape)
    p = p.astype(np.int64)
    h, w = p.shape[:2]
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    rs, gs, bs = (a.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) for a in (r, g, b))
    u = ((-38 * rs - 74 * gs + 112 * bs + 512) >> 10) + 128      # (numpy's >> on int64 floors, as an arithmetic shift does)
    v = ((112 * rs - 94 * gs - 18 * bs + 512) >> 10) + 128
    assert y.min() >= 16 and y.max() <= 235 and min(u.min(), v.min()) >= 16 and max(u.max(), v.max()) <= 240
    return yuv420ref.pack(y, u, v, fmt)

