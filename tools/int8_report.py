#!/usr/bin/env python3
"""The int8 pass's rate beside the fp16 and int16 passes of the same process (GPU box): frames/s at batches 64 and 256 with the frames
and region tensors resident in HBM, per-layer milliseconds of the int8 pass, and the share of the i8 matrix rate the pass reaches.
Writes profiles/r13_int8_rates.txt.  Each figure: 3 warm-up passes, then `steps` passes between two device synchronisations, host
clock.  usage: python3 tools/int8_report.py [steps = 10] [out = profiles/r13_int8_rates.txt]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, net, synth

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13_int8_rates.txt")
GOP_PER_FRAME = 2 * net.macs_per_frame() / 1e9          # 29.46
I8_PLANNING_OPS = 5.0e15                                 # "about 2x bf16" (~2.5 PF dense): a planning figure, not a measurement

dev = torch.device("cuda:0")
model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
ctx8 = hipdrv.Yolo2Hip(0)     # a context of its own: its per-layer events are not shared with the int16 / fp16 lanes of `ctx`
ctx8.load_model(ctx.calibrate_int8(frames=synth.frames(40, 4), batch=4))
base = synth.frames(7, 16)
st = torch.cuda.current_stream().cuda_stream
lines = [f"int8 pass beside fp16 and int16, one process, device-resident, {steps} timed passes after 3 warm-up passes", ""]


def rate(run, B):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)


fps = {}
for B in (64, 256):
    frames = torch.from_numpy(np.concatenate([base] * (B // 16))).to(dev)
    rf = torch.empty((B, 425, 13, 13), dtype=torch.float32, device=dev)
    ri = torch.empty((B, 425, 13, 13), dtype=torch.int16, device=dev)
    ctx.set_batch(B)
    fps[B] = {
        "int8": rate(lambda: ctx8.run_batch_int8_ptr(frames.data_ptr(), B, rf.data_ptr(), st), B),
        "fp16": rate(lambda: ctx.run_batch_fp16_ptr(frames.data_ptr(), B, rf.data_ptr(), st), B),
        "int16": rate(lambda: ctx.run_batch_ptr(frames.data_ptr(), B, ri.data_ptr(), st), B),
    }
    f = fps[B]
    lines.append(f"batch {B:3d}: int8 {f['int8']:9.0f} frames/s   fp16 {f['fp16']:9.0f}   int16 {f['int16']:9.0f}   "
                 f"int8 / int16 = {f['int8'] / f['int16']:.2f}   int8 / fp16 = {f['int8'] / f['fp16']:.2f}")
    if B == 256:
        ctx8.set_profiling(True)
        for _ in range(4):
            ctx8.run_batch_int8_ptr(frames.data_ptr(), B, rf.data_ptr(), st)
        torch.cuda.synchronize()
        ms = ctx8.layer_times_ms()
        ctx8.set_profiling(False)
    del frames, rf, ri

ops = fps[256]["int8"] * GOP_PER_FRAME * 1e9
lines += ["", f"int8 at batch 256: {ops / 1e12:.1f} TOP/s of the network's {GOP_PER_FRAME:.2f} GOP per frame = "
          f"{100 * ops / I8_PLANNING_OPS:.1f} % of the i8 planning figure ({I8_PLANNING_OPS / 1e15:.1f} POP/s dense, 2x bf16; not measured here)",
          f"condition (int8 >= 3x int16 at batch 256): {'met' if fps[256]['int8'] >= 3 * fps[256]['int16'] else 'NOT met'} "
          f"({fps[256]['int8'] / fps[256]['int16']:.2f}x)", "",
          "int8 pass, per-layer milliseconds at batch 256 (device events, mean of 4 passes):"]
for l in net.LAYERS:
    if l.type == net.REGION:
        continue
    gop = 2 * l.n * l.c * l.size * l.size * l.out_h * l.out_w * 256 / 1e9 if l.type == net.CONV else 0.0
    tail = f"   {gop / ms[l.idx]:8.1f} TOP/s" if gop and ms[l.idx] > 0 else ""
    lines.append(f"  layer {l.idx:2d} {l.type:5s} {ms[l.idx]:8.3f} ms{tail}")
lines.append(f"  sum {float(ms.sum()):8.3f} ms")
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
ctx8.close()
ctx.close()
