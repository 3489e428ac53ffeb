#!/usr/bin/env python3
"""What option jpeg_optimize costs and saves (GPU box): the annotate-and-encode entry and the fp16 camera loop with JPEG out at
768x576, quality 80, batch 256, in modes (subsample, restart) = (0, 0) and (420, 96), jpeg_optimize 0 against 1.  Frames and records
as tools/jpeg420_report.py: the dog frame rolled per frame, six records per frame.  One process; the settings alternate inside every
repeat; every figure is the median of the repeats with their spread (min .. max); stream bytes per frame beside it.
usage: python3 tools/jpeg_optimize_report.py [chunks per call = 2] [reps = 5]
       python3 tools/jpeg_optimize_report.py --bytes      (no GPU: the host encoder's stream bytes on the dog frame and the painted fixture)
       python3 tools/jpeg_optimize_report.py --trace <subsample> <restart> <optimize>   (two calls of the annotate entry at batch 64 in
                                        that setting and nothing else, for rocprofv3 --kernel-trace --stats -- python3 tools/... --trace ...)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
from yolo2_amd import hipdrv, synth

MODES = [(0, 0), (420, 96)]
QUALITY, THRESH, B = 80, 0.24, 256
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]
if len(sys.argv) > 1 and sys.argv[1] == "--bytes":
    painted = np.load(os.path.join(ROOT, "tests", "golden", "draw.npz"))
    key = max((k for k in painted.files if k.endswith("/paint")), key=lambda k: painted[k].size)      # the largest painted frame of the fixture
    frames = {"dog frame": DOG, f"painted fixture {key}": painted[key]}
    for name, im in frames.items():
        for m in MODES:
            std, opt = len(hipdrv.write_jpg_host(im, QUALITY, *m)), len(hipdrv.write_jpg_host(im, QUALITY, *m, optimize=True))
            print(f"{name} {im.shape[1]}x{im.shape[0]}, mode ({m[0]:3d}, {m[1]:2d}): {std} -> {opt} bytes ({opt / std:.4f})")
    sys.exit(0)

import torch
TRACE = len(sys.argv) > 1 and sys.argv[1] == "--trace"
CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 and not TRACE else 2
REPS = int(sys.argv[2]) if len(sys.argv) > 2 and not TRACE else 5
NAMES = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
torch.zeros(1, device="cuda:0")      # (a measurement path that finds no GPU fails here)
ctx = hipdrv.Yolo2Hip(0)
rng = np.random.default_rng(5)
base = [np.ascontiguousarray(np.roll(DOG, (37 * i, 53 * i), axis=(0, 1))) for i in range(16)]
rec = np.zeros((16, 8), dtype=hipdrv.DET_DTYPE)
for i in range(16):
    rec[i, :6]["cls"] = rng.integers(0, 80, 6)
    rec[i, :6]["prob"] = rng.uniform(.3, 1., 6)
    for k in ("x", "y"):
        rec[i, :6][k] = rng.uniform(.1, .9, 6)
    for k in ("w", "h"):
        rec[i, :6][k] = rng.uniform(.05, .5, 6)


def annotate(imgs, dets, counts, batch, s):
    return ctx.annotate_images(imgs, dets, counts, batch, THRESH, labels=NAMES, jpeg_quality=QUALITY, jpeg_subsample=s[0], jpeg_restart=s[1],
                               jpeg_optimize=s[2])[0]


if TRACE:
    s, n = tuple(int(v) for v in sys.argv[2:5]), 128
    for _ in range(2):
        annotate([base[i % 16] for i in range(n)], np.ascontiguousarray(rec[np.arange(n) % 16]), np.full(n, 6, dtype=np.int32), 64, s)
    ctx.close()
    sys.exit(0)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


n = CHUNKS * B
imgs = [base[i % 16] for i in range(n)]
dets, counts = np.ascontiguousarray(rec[np.arange(n) % 16]), np.full(n, 6, dtype=np.int32)
model = synth.SynthModel(seed=1, obj_bias=2.0)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
loop = lambda s: ctx.loop_images(imgs, precision="fp16", thresh=THRESH, labels=NAMES, jpeg_quality=QUALITY, batch=B, jpeg_subsample=s[0],
                                 jpeg_restart=s[1], jpeg_optimize=s[2])["frames"]
routes = [("annotate + encode entry", lambda s: annotate(imgs, dets, counts, B, s)), ("fp16 loop, JPEG out", loop)]
SETTINGS = [m + (o,) for m in MODES for o in (0, 1)]
print(f"# python3 tools/jpeg_optimize_report.py {CHUNKS} {REPS}   (one process, one MI355X; 768x576 dog frames rolled per frame, RGB24 in, quality "
      f"{QUALITY}, batch {B}, {n} frames per call; median of {REPS} repeats, the settings alternating inside a repeat (min .. max))")
for name, fn in routes:
    times, size = {s: [] for s in SETTINGS}, {}
    for s in SETTINGS:      # untimed: buffers, code objects
        size[s] = sum(len(d) for d in fn(s))
    for _ in range(REPS):
        for s in SETTINGS:
            times[s].append(clock(lambda: fn(s)))
    print(f"{name}:")
    med = lambda s: sorted(times[s])[len(times[s]) // 2]
    for s in SETTINGS:
        ts = sorted(times[s])
        print(f"    mode ({s[0]:3d}, {s[1]:2d}) optimize {s[2]}: {med(s) * 1e3:7.1f} ms per call = {n / med(s):6.0f} frames/s ({n / ts[-1]:.0f} .. {n / ts[0]:.0f}), "
              f"{size[s] / n:.0f} stream bytes per frame")
    for m in MODES:
        print(f"    mode ({m[0]}, {m[1]}): optimize 1 / 0 = {med(m + (0,)) / med(m + (1,)):.3f}x the rate at {size[m + (1,)] / size[m + (0,)]:.4f} of the bytes")
ctx.close()
