#!/usr/bin/env python3
"""Rate of the int8 images -> detections entry (yolo2_hip_run_images_pix_dets_int8: bytes in, k_i8_front_pix from the bytes to layer
1, layers 2..30, the float tail on the device, records out) beside the same entry under option i8_no_front (chunk letterbox + the
frames route) and the network-only int8 rate on resident frames, all in one process (GPU box).  Batches 64 and 256, 416x416 RGB24
and 768x576 YUYV.  Every figure: one warm-up call of the shape, then `reps` windows that end in a device synchronise; the two routes
alternate inside a repeat, and each repeat is printed so the spread shows.  Per chunk it prices what the entry overlaps (staging copy,
H2D, GPU).  From the context's per-layer events at batch 256 it sets the front kernel's time beside the launches it replaces.
Writes profiles/r14_int8_images_rates.txt.
usage: python3 tools/int8_images_report.py [chunks per call = 4] [reps = 3] [out = profiles/r14_int8_images_rates.txt]"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, synth

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r14_int8_images_rates.txt")
HBM_PEAK = 8.0e12            # bytes/s, MI355X data sheet (MI355X_MICROARCH.md); achievable copy rates are lower

dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
ctx.load_model(ctx.calibrate_int8(frames=synth.frames(40, 4), batch=4))
rng = np.random.default_rng(5)
lines = [f"int8 images -> records, fused front (k_i8_front_pix) beside option i8_no_front, one process; {CHUNKS} chunks per call, "
         f"{REPS} repeats after one warm-up call per shape, windows end in a device synchronise", ""]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def route(no_front):
    ctx.set_option("i8_no_front", 1 if no_front else None)


front_ms = {}
for B in (64, 256):
    frames = torch.from_numpy(np.concatenate([synth.frames(7, 16)] * (B // 16))).to(dev)
    region = torch.empty((B, 425, 13, 13), dtype=torch.float32, device=dev)
    net_run = lambda: ctx.run_batch_int8_ptr(frames.data_ptr(), B, region.data_ptr(), st)
    for _ in range(3):
        net_run()
    t_net = window(net_run, 8)
    say(f"batch {B}: network only (letterboxed fp32 frames resident in HBM, frames route): {t_net * 1e3:.2f} ms per chunk = {B / t_net:.0f} frames/s")
    if B == 256:       # per-layer events of the frames route: layers 0 and 1 are what the front replaces, with the letterbox and k_i8_quant_input
        ctx.set_profiling(True)
        for _ in range(4):
            net_run()
        torch.cuda.synchronize()
        ms_frames = ctx.layer_times_ms().copy()
        ctx.set_profiling(False)
    del frames, region
    for fmt, h, w in (("rgb24", 416, 416), ("yuyv", 576, 768)):
        ch = 3 if fmt == "rgb24" else 2
        base = [rng.integers(0, 256, (h, w, ch), dtype=np.uint8) for _ in range(16)]
        n = CHUNKS * B
        imgs = [base[i % 16] for i in range(n)]
        call = lambda: hipdrv.run_images_dets(ctx._h, imgs, B, 0.25, 0.45, cap=100, precision="int8", pixfmt=fmt)
        t = {False: [], True: []}
        for nf in (False, True):        # warm every shape on both routes
            route(nf)
            call()
        for _ in range(REPS):
            for nf in (False, True):
                route(nf)
                t[nf].append(window(call))
        route(False)
        call()
        name = ctx.images_front_kernel_int8()
        fused, unfused = min(t[False]), min(t[True])
        say(f"  {w}x{h} {fmt}: {n} images per call (chunks of {B})")
        say(f"    fused ({name}): best {fused * 1e3:.1f} ms = {n / fused:.0f} frames/s = {n / fused / (B / t_net):.2f} of the network-only rate; "
            f"all repeats {', '.join(f'{n / x:.0f}' for x in t[False])} frames/s")
        say(f"    i8_no_front: best {unfused * 1e3:.1f} ms = {n / unfused:.0f} frames/s; all repeats {', '.join(f'{n / x:.0f}' for x in t[True])} frames/s; "
            f"fused / i8_no_front = {unfused / fused:.2f}")
        nbytes = h * w * ch
        pinned = torch.empty(B * nbytes, dtype=torch.uint8).pin_memory()
        view = pinned.numpy()

        def stage():
            def part(k):
                for i in range(k, B, 4):
                    view[i * nbytes:(i + 1) * nbytes] = imgs[i].reshape(-1)
            with ThreadPoolExecutor(4) as ex:
                list(ex.map(part, range(4)))
        stage()
        t0 = time.perf_counter()
        for _ in range(REPS):
            stage()
        t_stage = (time.perf_counter() - t0) / REPS
        dbuf = torch.empty(B * nbytes, dtype=torch.uint8, device=dev)
        dbuf.copy_(pinned, non_blocking=True)
        t_h2d = window(lambda: dbuf.copy_(pinned, non_blocking=True), 8)
        del dbuf, pinned
        say(f"    per chunk: staging copy {t_stage * 1e3:.2f} ms ({B * nbytes / t_stage / 1e9:.1f} GB/s, 4 threads), H2D {t_h2d * 1e3:.2f} ms "
            f"({B * nbytes / t_h2d / 1e9:.1f} GB/s), GPU (network only) {t_net * 1e3:.2f} ms; call / chunk {fused / CHUNKS * 1e3:.2f} ms")
        if B == 256:       # the front kernel's own time: layer 1's slot of the events on the fused route, one chunk per call
            one = imgs[:B]
            ctx.set_profiling(True)
            for _ in range(4):
                ctx.run_images_int8_host(one, B, pixfmt=fmt)
            torch.cuda.synchronize()
            ms = ctx.layer_times_ms().copy()
            ctx.set_profiling(False)
            front_ms[fmt] = (float(ms[1]), float(ms[0]), float(ms.sum()), nbytes)

say()
say("front kernel at batch 256 (device events, mean of 4 passes; the fused route's time is in layer 1's slot, layer 0's slot is empty):")
l0, l1 = float(ms_frames[0]), float(ms_frames[1])
say(f"  frames route: layer 0 (k_conv_i8, nine k steps) {l0:.3f} ms + layer 1 (k_i8_pool) {l1:.3f} ms = {l0 + l1:.3f} ms; sum of all slots "
    f"{float(ms_frames.sum()):.3f} ms.  The chunk letterbox and k_i8_quant_input run in front of the first event and are in no slot: "
    f"{l0 + l1:.3f} ms is a LOWER bound of what the front kernel replaces.")
for fmt, (f_ms, slot0, total, nbytes) in front_ms.items():
    algo = 256 * (nbytes + 208 * 208 * 32)
    say(f"  {fmt}: front kernel {f_ms:.3f} ms (layer 0's slot {slot0:.3f} ms, all slots {total:.3f} ms) = {f_ms / (l0 + l1):.2f} of layers 0 + 1 of "
        f"the frames route; algorithmic bytes {algo / 1e6:.0f} MB (image bytes read + 208*208*32 written per frame) = "
        f"{algo / (f_ms * 1e-3) / 1e12:.2f} TB/s of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
if "rgb24" in front_ms:
    ok = front_ms["rgb24"][0] < l0 + l1
    say(f"condition (batch 256, 416x416 RGB24: front kernel below the launches it replaces): {'met' if ok else 'NOT met'} "
        f"({front_ms['rgb24'][0]:.3f} ms against at least {l0 + l1:.3f} ms)")
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
ctx.close()
