#!/usr/bin/env python3
"""Rates of the JPEG encoder's modes (GPU box): the annotate-and-encode entry (yolo2_hip_annotate_images_pix_jpeg_host, RGB24 frames
in) and the fp16 camera loop with JPEG out (yolo2_hip_loop_images_pix) at 768x576, quality 80, batch 256, in modes (subsample,
restart) = (0, 0), (420, 0) and (420, 96) - 96 MCUs are two MCU rows of a 768-wide 4:2:0 frame.  Frames and records as
tools/jpeg_report.py: the dog frame rolled per frame, six records per frame.  One process; the modes alternate inside every repeat;
every figure is the median of the repeats with their spread (min .. max); stream bytes per frame beside it.
usage: python3 tools/jpeg420_report.py [chunks per call = 2] [reps = 5]
       python3 tools/jpeg420_report.py --trace <subsample> <restart>   (two calls of the annotate entry at batch 64 in that mode and
                                        nothing else, for rocprofv3 --kernel-trace --stats -- python3 tools/jpeg420_report.py --trace ...)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, synth

TRACE = len(sys.argv) > 1 and sys.argv[1] == "--trace"
CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 and not TRACE else 2
REPS = int(sys.argv[2]) if len(sys.argv) > 2 and not TRACE else 5
MODES = [(0, 0), (420, 0), (420, 96)]
QUALITY, THRESH, B = 80, 0.24, 256
NAMES = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]
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


def annotate(imgs, dets, counts, batch, mode):
    return ctx.annotate_images(imgs, dets, counts, batch, THRESH, labels=NAMES, jpeg_quality=QUALITY, jpeg_subsample=mode[0], jpeg_restart=mode[1])[0]


if TRACE:
    mode, n = (int(sys.argv[2]), int(sys.argv[3])), 128
    for _ in range(2):
        annotate([base[i % 16] for i in range(n)], np.ascontiguousarray(rec[np.arange(n) % 16]), np.full(n, 6, dtype=np.int32), 64, mode)
    ctx.close()
    sys.exit(0)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def line(name, n, ts, nbytes):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return f"    {name}: {med * 1e3:7.1f} ms per call = {n / med:6.0f} frames/s ({n / ts[-1]:.0f} .. {n / ts[0]:.0f}), {nbytes / n:.0f} stream bytes per frame"


n = CHUNKS * B
imgs = [base[i % 16] for i in range(n)]
dets, counts = np.ascontiguousarray(rec[np.arange(n) % 16]), np.full(n, 6, dtype=np.int32)
model = synth.SynthModel(seed=1, obj_bias=2.0)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
loop = lambda mode: ctx.loop_images(imgs, precision="fp16", thresh=THRESH, labels=NAMES, jpeg_quality=QUALITY, batch=B, jpeg_subsample=mode[0],
                                    jpeg_restart=mode[1])["frames"]
routes = [("annotate + encode entry", lambda mode: annotate(imgs, dets, counts, B, mode)), ("fp16 loop, JPEG out     ", loop)]
print(f"# python3 tools/jpeg420_report.py {CHUNKS} {REPS}   (one process, one MI355X; 768x576 dog frames rolled per frame, RGB24 in, quality {QUALITY}, "
      f"batch {B}, {n} frames per call; median of {REPS} repeats, the modes alternating inside a repeat (min .. max))")
for name, fn in routes:
    times, size = {m: [] for m in MODES}, {}
    for m in MODES:      # untimed: buffers, code objects
        size[m] = sum(len(s) for s in fn(m))
    for _ in range(REPS):
        for m in MODES:
            times[m].append(clock(lambda: fn(m))[0])
    print(f"{name.strip()}:")
    for m in MODES:
        print(line(f"mode ({m[0]:3d}, {m[1]:2d})", n, times[m], size[m]))
    med = lambda m: sorted(times[m])[len(times[m]) // 2]
    print(f"    (420, 0) / (0, 0) = {med(MODES[0]) / med(MODES[1]):.2f}x the rate at {size[MODES[1]] / size[MODES[0]]:.2f} of the bytes; "
          f"(420, 96) / (420, 0) = {med(MODES[1]) / med(MODES[2]):.2f}x the rate")
ctx.close()
