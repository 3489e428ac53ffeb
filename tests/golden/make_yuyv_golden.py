#!/usr/bin/env python3
"""Generate tests/golden/yuyv.npz from the REFERENCE's own YUYV -> RGB24 conversion.

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_yuyv_golden.py

The reference's camera loop (linux_app/src/main.c:942-984) turns a V4L2 YUYV frame into RGB24 with yolo2_yuyv_to_rgb24
(linux_app/src/yolo2_v4l2.c:328-374).  This script compiles that translation unit from the reference's sources into a temporary
directory OUTSIDE the repository, calls the function, and stores only data: a few small YUYV frames with the RGB the reference
made of them, and the sha256 of its output over all 2^24 (Y, U, V) triples.  tests/test_yuyv_host.py pins y2h_yuyv_to_rgb24 to both;
the GPU tests take their expected values from the RGB entries fed this conversion.
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_APP = "/root/reference/linux_app"
# measured from the compiled reference; the generator refuses to write the fixture unless it reproduces this value
EXHAUSTIVE_SHA256 = "aa952659e845ecb743186daf48be932e6c6d584a072f2d367ef85242d18d2b4f"


def build_reference(tmp):
    so = os.path.join(tmp, "libref_v4l2.so")
    src = [os.path.join(REF_APP, "src", f) for f in ("yolo2_v4l2.c", "stb_image_impl.c", "yolo2_log.c")]
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I" + os.path.join(REF_APP, "include"),
                    "-I" + os.path.join(REF_APP, "include", "third_party"), "-o", so] + src + ["-lm"], check=True)
    lib = C.CDLL(so)
    lib.yolo2_yuyv_to_rgb24.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.yolo2_yuyv_to_rgb24.restype = None
    return lib


def ref_convert(lib, yuyv):
    """yuyv uint8 [h][w][2] -> the reference's RGB24 uint8 [h][w][3]"""
    yuyv = np.ascontiguousarray(yuyv, dtype=np.uint8)
    h, w = yuyv.shape[:2]
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    lib.yolo2_yuyv_to_rgb24(yuyv.ctypes.data, rgb.ctypes.data, w, h)
    return rgb


def exhaustive_frame(y):
    """512 x 256 frame whose pairs are (y, u, 255 - y, v), u = row, v = pair within the row: with y = 0..255 every (Y, U, V) triple"""
    f = np.empty((256, 256, 4), dtype=np.uint8)
    f[:, :, 0] = y
    f[:, :, 1] = np.arange(256, dtype=np.uint8)[:, None]
    f[:, :, 2] = 255 - y
    f[:, :, 3] = np.arange(256, dtype=np.uint8)[None, :]
    return f.reshape(256, 512, 2)


def rgb_to_yuyv(rgb):
    """a natural YUYV frame from an RGB image (BT.601 studio range, chroma of the pair's mean); only an INPUT, so any sensible
    conversion serves"""
    p = rgb.astype(np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 16 + (65.738 * r + 129.057 * g + 25.064 * b) / 256
    u = 128 + (-37.945 * r - 74.494 * g + 112.439 * b) / 256
    v = 128 + (112.439 * r - 94.154 * g - 18.285 * b) / 256
    h, w = y.shape
    out = np.empty((h, w, 2), dtype=np.uint8)
    out[..., 0] = np.clip(np.rint(y), 0, 255)
    out[:, 0::2, 1] = np.clip(np.rint((u[:, 0::2] + u[:, 1::2]) / 2), 0, 255)
    out[:, 1::2, 1] = np.clip(np.rint((v[:, 0::2] + v[:, 1::2]) / 2), 0, 255)
    return out


def main():
    if not os.path.isdir(REF_APP):
        sys.exit("needs the reference tree at /root/reference")
    with tempfile.TemporaryDirectory(prefix="y2_yuyv_ref_") as tmp:
        assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)) + os.sep)
        lib = build_reference(tmp)
        sha = hashlib.sha256()
        for y in range(256):
            sha.update(ref_convert(lib, exhaustive_frame(y)).tobytes())
        if sha.hexdigest() != EXHAUSTIVE_SHA256:
            sys.exit(f"the compiled reference gives sha256 {sha.hexdigest()} over all (Y, U, V) triples, not the recorded {EXHAUSTIVE_SHA256}")
        rng = np.random.default_rng(20261016)
        dog = np.load(os.path.join(HERE, "dog.npz"))["rgb"]
        frames = {
            "random_32x24": rng.integers(0, 256, (24, 32, 2), dtype=np.uint8),     # all three clamps fire both ways
            "random_2x1": rng.integers(0, 256, (1, 2, 2), dtype=np.uint8),
            "random_2x2": rng.integers(0, 256, (2, 2, 2), dtype=np.uint8),
            "random_6x5": rng.integers(0, 256, (5, 6, 2), dtype=np.uint8),
            "dog_64x48": rgb_to_yuyv(dog[150:150 + 48 * 6:6, 200:200 + 64 * 6:6]),
        }
        out = {"exhaustive_sha256": np.frombuffer(bytes.fromhex(EXHAUSTIVE_SHA256), dtype=np.uint8)}
        for name, f in frames.items():
            out[name + "/yuyv"] = f
            out[name + "/rgb"] = ref_convert(lib, f)
        r = out["random_32x24/rgb"]
        assert (r == 0).any(axis=(0, 1)).all() and (r == 255).any(axis=(0, 1)).all(), "the random frame must clamp every channel both ways"
    path = os.path.join(HERE, "yuyv.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(frames)} frames, exhaustive sha256 {EXHAUSTIVE_SHA256}")


if __name__ == "__main__":
    main()
