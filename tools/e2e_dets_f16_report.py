#!/usr/bin/env python3
"""Rate of the images -> detections entry on the matrix-core passes (yolo2_hip_run_images_u8_dets_f16: bytes in, layers 0+1 straight
from the bytes, network, region / boxes / NMS on the device, records out), next to the device-resident rate of the network alone on
letterboxed frames, in one process (GPU box).  fp16 at batch 256 and split-fp16 at batch 128, 416x416 and 768x576 RGB images.
Per chunk it also prices the stages the entry overlaps: the staging copy (pageable images -> pinned buffer, the entry's four
threads), the H2D of the chunk's bytes (pinned, one DMA) and the GPU work (the network-only pass).
usage: python3 tools/e2e_dets_f16_report.py [chunks per call = 8] [reps = 3]"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, synth

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
rng = np.random.default_rng(5)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for precision, B in (("fp16", 256), ("fp32fast", 128)):
    split = precision == "fp32fast"
    frames = torch.from_numpy(synth.frames(7, B)).to(dev)
    region = torch.empty((B, 425, 13, 13), dtype=torch.float32, device=dev)
    run = ctx.run_batch_f32tol_ptr if split else ctx.run_batch_fp16_ptr
    t_net = timed(lambda: run(frames.data_ptr(), B, region.data_ptr(), st), 8)
    print(f"{precision} batch {B}: network only (letterboxed fp32 frames resident in HBM): {t_net * 1e3:.2f} ms per chunk = {B / t_net:.0f} frames/s")
    del frames, region
    for h, w in ((416, 416), (576, 768)):
        base = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(16)]
        n = CHUNKS * B
        imgs = [base[i % 16] for i in range(n)]
        t_call = timed(lambda: hipdrv.run_images_dets(ctx._h, imgs, B, 0.25, 0.45, cap=100, precision=precision), REPS)
        # the stages of one chunk, each alone
        nbytes = h * w * 3
        pinned = torch.empty(B * nbytes, dtype=torch.uint8).pin_memory()
        view = pinned.numpy()
        def stage():
            def part(t):
                for i in range(t, B, 4):
                    view[i * nbytes:(i + 1) * nbytes] = imgs[i].reshape(-1)
            with ThreadPoolExecutor(4) as ex:
                list(ex.map(part, range(4)))
        t0 = time.perf_counter()
        for _ in range(REPS):
            stage()
        t_stage = (time.perf_counter() - t0) / REPS
        dbuf = torch.empty(B * nbytes, dtype=torch.uint8, device=dev)
        t_h2d = timed(lambda: dbuf.copy_(pinned, non_blocking=True), 8)
        del dbuf, pinned
        print(f"  {w}x{h}: images -> records {n} images per call (chunks of {B}): {t_call * 1e3:.1f} ms per call = {n / t_call:.0f} frames/s "
              f"= {n / t_call / (B / t_net):.2f} of the network-only rate; layer 0: {ctx.images_layer0_kernel(split)}")
        print(f"           per chunk: staging copy {t_stage * 1e3:.2f} ms ({B * nbytes / t_stage / 1e9:.1f} GB/s, 4 threads), "
              f"H2D {t_h2d * 1e3:.2f} ms ({B * nbytes / t_h2d / 1e9:.1f} GB/s), GPU (network only) {t_net * 1e3:.2f} ms; "
              f"call / chunk {t_call / CHUNKS * 1e3:.2f} ms")
ctx.close()
