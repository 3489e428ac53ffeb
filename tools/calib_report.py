#!/usr/bin/env python3
"""What calibration buys and costs, measured on the GPU (profiles/r08_calibration.txt):
  A. error of the int16 region tensor against the exact fp32 pass, frames 0 (calibrated on) and 1 (held out), with the hand-picked
     STD_Q tables, with only the activation tables calibrated, and with the full rule (weights, biases, activations);
  B. tests/f16models.DenseModel (full-mantissa fp32 weights, per-channel spread): region error and box IoU against fp32;
  C. calibration frames/s at batch 32 beside the exact fp32 pass's own rate in the same process;
  D. the int16 pass's rate and arithmetic forms per 32-channel block with calibrated tables beside STD_Q's.
usage: python3 tools/calib_report.py [out.txt]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import bench                                    # box_iou_vs_reference: the comparison behind box_iou_vs_fp32_oracle
import f16models
from yolo2_amd import hipdrv, net, synth

NCONV = len(net.CONVS)
OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def errors(region_i16, q, exact):
    e = region_i16.astype(np.float64) * 2.0 ** -q - exact
    return float(np.abs(e).max()), float(np.sqrt((e ** 2).mean()))


def sync():
    b = hipdrv.DevBuf(nbytes=16)
    b.get(np.uint8, (16,))
    b.free()


def rate(fn, frames_per_step, steps, warmup=2):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return frames_per_step * steps / (time.perf_counter() - t0)


class ActOnly:
    """the synthetic model's own int16 weights and weight / bias tables with calibrated activation tables"""

    def __init__(self, model, act_q):
        self.weights_i16, self.bias_i16 = model.weights_i16, model.bias_i16
        self.weight_q, self.bias_q, self.act_q = model.weight_q, model.bias_q, np.array(act_q, dtype=np.int32)


def main():
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    frames = synth.frames(1, 2)
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    cal = ctx.calibrate(frames=frames[:1], batch=1)
    exact = ctx.run_batch_fp32_host(frames)
    say("# calibration: fp32 weights + frames -> int16 weights and Q tables (tools/calib_report.py)")
    say()
    say("## A. SynthModel(seed=1, obj_bias=2.0), calibrated on synth.frames(1, 2)[0], headroom 1")
    say(f"act_absmax  {[float('%.5g' % v) for v in cal.act_absmax]}")
    say(f"act_q       {list(map(int, cal.act_q))}   (STD_Q: 14, then 9)")
    say(f"weight_q    {list(map(int, cal.weight_q))}   (STD_Q: 14)")
    say(f"bias_q      {list(map(int, cal.bias_q))}   (STD_Q: 12)")
    say(f"values clamped by the quantiser: {cal.clamped}")
    say("max abs / rms error of the dequantised int16 region tensor against the exact fp32 pass's:")
    say("| tables | frame 0 (calibrated on) max | rms | frame 1 (held out) max | rms |")
    say("|---|---|---|---|---|")
    runs = {}
    for tag, m in (("STD_Q (hand-picked)", model), ("activation Q calibrated only", ActOnly(model, cal.act_q)), ("full rule", cal)):
        c = hipdrv.Yolo2Hip(0)
        c.load_model(m)
        region, q = c.run_batch_host(frames)
        runs[tag] = [errors(region[f], q, exact[f]) for f in range(2)]
        c.close()
        (a, b), (d, e) = runs[tag]
        say(f"| {tag} | {a:.4f} | {b:.4f} | {d:.4f} | {e:.4f} |")
    worse = [f for f in range(2) if runs["full rule"][f][0] > runs["activation Q calibrated only"][f][0]]
    say("full rule against activations only: " + (f"WORSE in max abs error on frame(s) {worse}" if worse else "not worse on either frame") +
        " (SynthModel's fp32 weights are int16 x 2^-14 and its biases int16 x 2^-12, so any Q that holds them represents them exactly)")
    say()

    say("## B. DenseModel (full-mantissa fp32 weights; no int16 form before), calibrated on frame 0, measured on frame 0")
    base = synth.SynthModel(seed=1)
    for spread in (0.5, 3.0):
        dense = f16models.DenseModel(seed=1, spread=spread, base=base)
        ctx.load_weights_fp32(dense.weights_f32(), dense.bias_f32())
        dcal = ctx.calibrate(frames=frames[:1], batch=1)
        dexact = ctx.run_batch_fp32_host(frames[:1])[0]
        c = hipdrv.Yolo2Hip(0)
        c.load_model(dcal)
        region, q = c.run_batch_host(frames[:1])
        c.close()
        mx, rms = errors(region[0], q, dexact)
        iou = bench.box_iou_vs_reference(region[0].astype(np.float32) * np.float32(2.0 ** -q), dexact)
        say(f"spread {spread}: act_q {list(map(int, dcal.act_q))}")
        say(f"            weight_q {list(map(int, dcal.weight_q))} bias_q {list(map(int, dcal.bias_q))} clamped {dcal.clamped}")
        say(f"            region error vs fp32: max {mx:.4f} rms {rms:.4f} (region spans +-{np.abs(dexact).max():.2f}); boxes: IoU min {iou['box_iou_min']:.4f} "
            f"mean {iou['box_iou_mean']:.4f}, confident ({iou['confident_boxes']}) IoU min {iou['confident_box_iou_min']}, max coord err {iou['max_abs_coord_err']:.5f}, "
            f"max objectness err {iou['max_abs_objectness_err']:.5f}")
    say()

    say("## C. calibration rate, batch 32 (frames resident in HBM; alternating, three repeats)")
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    B = 32
    fr = hipdrv.DevBuf(synth.frames(3, B))
    reg = hipdrv.DevBuf(nbytes=B * 425 * 169 * 4)
    L = hipdrv.lib()
    ctx.calib_reset()
    for rep in range(3):
        r_pass = rate(lambda: ctx.run_batch_fp32_ptr(fr.addr, B, reg.addr), B, 6)
        r_cal = rate(lambda: hipdrv.check(L.yolo2_hip_calib_frames(ctx._h, fr.addr, B, None), "calib_frames"), B, 6)
        say(f"repeat {rep}: exact fp32 pass {r_pass:.0f} frames/s   yolo2_hip_calib_frames {r_cal:.0f} frames/s   ({r_cal / r_pass:.3f} of the pass: "
            f"the look at the frames, 24 reductions, two stream synchronisations and the region buffer per call)")
    t0 = time.perf_counter()
    ctx.calib_q_tables(1.0)
    t1 = time.perf_counter()
    ctx.quantize_weights(cal.weight_q, cal.bias_q)
    t2 = time.perf_counter()
    say(f"yolo2_hip_calib_q_tables (46 weight / bias reductions + the rule): {1e3 * (t1 - t0):.1f} ms;  yolo2_hip_quantize_weights_int16 "
        f"(46 launches + 102 MB back to the host): {1e3 * (t2 - t1):.1f} ms")
    fr.free()
    reg.free()
    say()

    say("## D. the int16 pass with calibrated tables beside STD_Q, batch 64 (alternating, three repeats)")
    B = 64
    fr = hipdrv.DevBuf(synth.frames(7, B))
    reg = hipdrv.DevBuf(nbytes=B * 425 * 169 * 2)
    ctxs = {}
    for tag, m in (("STD_Q", model), ("calibrated", cal)):
        c = hipdrv.Yolo2Hip(0)
        c.load_model(m)
        c.set_batch(B)
        ctxs[tag] = c
        say(f"{tag}: plan source {c.plan_source()}, lanes {c.num_lanes()}, forms per layer {c.layer_paths()}")
        say(f"{tag}: blocks per form [A, B, 64-bit, C, D] per conv layer {c.layer_path_counts()}")
    for rep in range(3):
        r = {tag: rate(lambda c=c: c.run_batch_ptr(fr.addr, B, reg.addr), B, 20, warmup=3) for tag, c in ctxs.items()}
        say(f"repeat {rep}: STD_Q {r['STD_Q']:.0f} frames/s   calibrated {r['calibrated']:.0f} frames/s")
    for c in ctxs.values():
        c.close()
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
