#!/usr/bin/env python3
"""Rate of annotated frames as JPEG streams (GPU box): yolo2_hip_annotate_images_pix_jpeg_host at 768x576, quality 80, from YUYV and
from RGB24 frames, batches 64 and 256, against (a) the RGB24 annotate entry on the same frames (yolo2_hip_annotate_images_pix_host:
3 bytes per pixel come back) and (b) that entry followed by y2h_write_jpg_rgb24 on four host threads - what a user of the RGB24
entry does to get the reference's stream.  Frames: the dog frame of tests/golden/dog.npz rolled by a different offset per frame, so
the streams' sizes differ (random bytes barely compress and are no JPEG workload); six records per frame.  One process; the routes
alternate; every figure is the median of the repeats with their spread (min .. max).  Also: mean bytes per frame, and - as
stand-ins taken outside the entry, since it does not time its own streams - a bare pinned D2H of one chunk's stream bytes and a
host copy of them, as shares of the entry's time per chunk.
usage: python3 tools/jpeg_report.py [chunks per call = 4] [reps = 5] [tree]
       python3 tools/jpeg_report.py --trace      (two calls of the entry at batch 64 and nothing else, for
                                                  rocprofv3 --kernel-trace --stats -- python3 tools/jpeg_report.py --trace)"""
import ctypes as C
import os, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv

TRACE = len(sys.argv) > 1 and sys.argv[1] == "--trace"
CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 and not TRACE else 4
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
TREE = sys.argv[3] if len(sys.argv) > 3 else ""
THREADS, QUALITY, THRESH = 4, 80, 0.24
W, H = 768, 576
dev = torch.device("cuda:0")
NAMES = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]
ctx = hipdrv.Yolo2Hip(0)
pool = ThreadPoolExecutor(THREADS)
H_LIB = hipdrv.host_lib()


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def clock(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fmt_rate(n, ts):
    med, lo, hi = spread(ts)
    return f"{med * 1e3:.1f} ms per call = {n / med:.0f} frames/s ({n / hi:.0f} .. {n / lo:.0f})"


def to_yuyv(rgb):
    """BT.601 studio-range YUYV of an RGB frame (the report's camera frames; the entries convert them back on the GPU)"""
    r, g, b = (rgb[:, :, k].astype(np.float32) for k in range(3))
    y = np.clip(np.rint(16 + .257 * r + .504 * g + .098 * b), 0, 255)
    u = np.clip(np.rint(128 - .148 * r - .291 * g + .439 * b), 0, 255)
    v = np.clip(np.rint(128 + .439 * r - .368 * g - .071 * b), 0, 255)
    out = np.empty((rgb.shape[0], rgb.shape[1], 2), dtype=np.uint8)
    out[:, :, 0] = y
    out[:, 0::2, 1] = u[:, 0::2]
    out[:, 1::2, 1] = v[:, 0::2]
    return out


def tree():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD^{tree}"], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
        return head + (" + uncommitted changes" if dirty else "") if head else "unknown"
    except OSError:
        return "unknown"


rng = np.random.default_rng(5)
base_rgb = [np.ascontiguousarray(np.roll(DOG, (37 * i, 53 * i), axis=(0, 1))) for i in range(16)]
base_yuyv = [to_yuyv(im) for im in base_rgb]
rec = np.zeros((16, 8), dtype=hipdrv.DET_DTYPE)
for i in range(16):
    rec[i, :6]["cls"] = rng.integers(0, 80, 6)
    rec[i, :6]["prob"] = rng.uniform(.3, 1., 6)
    for k in ("x", "y"):
        rec[i, :6][k] = rng.uniform(.1, .9, 6)
    for k in ("w", "h"):
        rec[i, :6][k] = rng.uniform(.05, .5, 6)

if TRACE:
    n = 128
    imgs = [base_yuyv[i % 16] for i in range(n)]
    dets = np.ascontiguousarray(rec[np.arange(n) % 16])
    for _ in range(2):
        ctx.annotate_images(imgs, dets, np.full(n, 6, dtype=np.int32), 64, THRESH, labels=NAMES, pixfmt="yuyv", jpeg_quality=QUALITY)
    ctx.close()
    sys.exit(0)

print(f"# python3 tools/jpeg_report.py {CHUNKS} {REPS}   (one process, one MI355X; {W}x{H} dog frames rolled per frame, 6 records per frame at thresh "
      f"{THRESH}, quality {QUALITY}; median of {REPS} alternating repeats (min .. max); tree {TREE or tree()})")
for B in (64, 256):
    n = CHUNKS * B
    dets = np.ascontiguousarray(rec[np.arange(n) % 16])
    counts = np.full(n, 6, dtype=np.int32)
    for pixfmt, base in (("yuyv", base_yuyv), ("rgb24", base_rgb)):
        imgs = [base[i % 16] for i in range(n)]
        jpg = lambda: ctx.annotate_images(imgs, dets, counts, B, THRESH, labels=NAMES, pixfmt=pixfmt, jpeg_quality=QUALITY)
        anno = lambda: ctx.annotate_images(imgs, dets, counts, B, THRESH, labels=NAMES, pixfmt=pixfmt)
        streams, drawn = jpg()              # untimed: buffers
        frames, _ = anno()
        mean_bytes = sum(len(s) for s in streams) / n
        bound = hipdrv.jpeg_bound(W, H)
        scratch = [np.empty(bound, dtype=np.uint8) for _ in range(THREADS)]

        def host_encode(frames):
            def part(t):
                for i in range(t, n, THREADS):
                    H_LIB.y2h_write_jpg_rgb24(frames[i].ctypes.data, W, H, QUALITY, scratch[t].ctypes.data, bound)
            list(pool.map(part, range(THREADS)))
        t_j, t_a, t_ah = [], [], []
        for _ in range(REPS):
            t_j.append(clock(jpg))
            t_a.append(clock(anno))
            t_ah.append(clock(lambda: host_encode(anno()[0])))
        j = spread(t_j)[0]
        print(f"batch {B}, {pixfmt}, {n} frames per call, {drawn.mean():.1f} records drawn per frame, {mean_bytes:.0f} stream bytes per frame "
              f"({W * H * 3 / mean_bytes:.1f}x fewer than RGB24):")
        print(f"    jpeg entry (bytes -> JPEG streams on the host):            {fmt_rate(n, t_j)}")
        print(f"    (a) RGB24 annotate entry:                                  {fmt_rate(n, t_a)}  -> jpeg entry / (a) = {spread(t_a)[0] / j:.2f}x")
        print(f"    (b) RGB24 annotate entry, then host encode on {THREADS} threads:   {fmt_rate(n, t_ah)}  -> jpeg entry / (b) = {spread(t_ah)[0] / j:.2f}x")
        # stand-ins, taken outside the entry with torch / numpy copies of as many bytes as one chunk's streams: what the entry's own
        # download and copy out of pinned memory cost at least (the entry does not time its streams)
        chunk_bytes = int(mean_bytes * B)
        pinned = torch.empty(chunk_bytes, dtype=torch.uint8).pin_memory()
        dbuf = torch.zeros(chunk_bytes, dtype=torch.uint8, device=dev)
        clock(lambda: pinned.copy_(dbuf, non_blocking=True))
        d2h = spread([clock(lambda: pinned.copy_(dbuf, non_blocking=True)) for _ in range(9)])
        src, dst = pinned.numpy(), np.empty(chunk_bytes, dtype=np.uint8)
        cp = spread([clock(lambda: np.copyto(dst, src)) for _ in range(9)])
        per_chunk = j / CHUNKS
        share = lambda t: f"{t[0] * 1e3:.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f}) = {t[0] / per_chunk:.3f} ({t[1] / per_chunk:.3f} .. {t[2] / per_chunk:.3f}) of the entry's time per chunk"
        print(f"    stand-ins for one chunk's streams ({chunk_bytes / 1e6:.1f} MB), median of 9 (min .. max): bare pinned D2H {share(d2h)};")
        print(f"        host copy out of pinned memory {share(cp)}")
        del imgs, streams, frames, pinned, dbuf
ctx.close()
