#!/usr/bin/env python3
"""Rate of YUYV camera frames -> detection records (GPU box): the _pix_dets entries reading the YUYV bytes on the GPU
(yolo2_hip_run_images_pix_dets[_f16] with YOLO2_PIX_YUYV) against the route a caller had without them, on the same frames: convert
every frame to RGB24 on host threads (y2h_yuyv_to_rgb24, on as many threads as the entries' staging copy uses), then the RGB entry
(yolo2_hip_run_images_u8_dets[_f16]).  fp16 at batch 256 and int16 at batch 64, 640x480 and 768x576, one process; the two routes
alternate and every figure is the median of the repeats with their spread (min .. max).  Per chunk it also prices, for both formats,
the stages the entries overlap: staging copy (pageable -> pinned, four threads), H2D of the chunk's bytes, GPU (network only).
usage: python3 tools/e2e_dets_yuyv_report.py [chunks per call = 8] [reps = 5]"""
import ctypes as C
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, synth

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
THREADS = 4     # kStageThreads of the entries' staging copy
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
host = C.CDLL(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "libyolo2_host.so"))
host.y2h_yuyv_to_rgb24.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
rng = np.random.default_rng(5)
pool = ThreadPoolExecutor(THREADS)


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


def chunk_stages(imgs, B):
    """(staging copy, H2D) seconds of one chunk of B frames, each alone, medians"""
    nbytes = imgs[0].nbytes
    pinned = torch.empty(B * nbytes, dtype=torch.uint8).pin_memory()
    view = pinned.numpy()
    def part(t):
        for i in range(t, B, THREADS):
            view[i * nbytes:(i + 1) * nbytes] = imgs[i].reshape(-1)
    t_stage = spread([clock(lambda: list(pool.map(part, range(THREADS)))) for _ in range(REPS)])[0]
    dbuf = torch.empty(B * nbytes, dtype=torch.uint8, device=dev)
    dbuf.copy_(pinned, non_blocking=True)
    torch.cuda.synchronize()
    t_h2d = spread([clock(lambda: dbuf.copy_(pinned, non_blocking=True)) for _ in range(8)])[0]
    return t_stage, t_h2d, nbytes


print(f"# python3 tools/e2e_dets_yuyv_report.py {CHUNKS} {REPS}   (one process, one MI355X; synthetic weights SynthModel(seed=1), random YUYV frames; "
      f"median of {REPS} alternating repeats (min .. max))")
for precision, B in (("fp16", 256), ("int16", 64)):
    frames = torch.from_numpy(synth.frames(7, B)).to(dev)
    if precision == "fp16":
        region = torch.empty((B, 425, 13, 13), dtype=torch.float32, device=dev)
        net = lambda: ctx.run_batch_fp16_ptr(frames.data_ptr(), B, region.data_ptr(), st)
    else:
        ctx.set_batch(B)
        region = torch.empty((B, 425, 13, 13), dtype=torch.int16, device=dev)
        net = lambda: ctx.run_batch_ptr(frames.data_ptr(), B, region.data_ptr(), st)
    clock(net)
    t_net = spread([clock(net) for _ in range(8)])[0]
    print(f"{precision} batch {B}: network only (letterboxed fp32 frames resident in HBM): {t_net * 1e3:.2f} ms per chunk = {B / t_net:.0f} frames/s")
    del frames, region
    for h, w in ((480, 640), (576, 768)):
        base = [rng.integers(0, 256, (h, w, 2), dtype=np.uint8) for _ in range(16)]
        n = CHUNKS * B
        yuyv = [base[i % 16] for i in range(n)]
        rgb = [np.empty((h, w, 3), dtype=np.uint8) for _ in range(n)]       # a converted copy per frame, as a caller's loop makes them
        def convert():
            def part(t):
                for i in range(t, n, THREADS):
                    host.y2h_yuyv_to_rgb24(yuyv[i].ctypes.data, rgb[i].ctypes.data, w, h)
            list(pool.map(part, range(THREADS)))
        dets = lambda imgs, pixfmt: hipdrv.run_images_dets(ctx._h, imgs, B, 0.25, 0.45, cap=100, precision=precision, pixfmt=pixfmt)
        convert()
        a = dets(yuyv, "yuyv")                              # untimed: buffers, plans; and the records agree
        l0 = ctx.images_layer0_kernel(False) if precision == "fp16" else "k_letterbox_yuyv_batch + the int16 table"
        b = dets(rgb, None)
        assert np.array_equal(a["counts"], b["counts"]) and all(np.array_equal(x, y) for x, y in zip(a["dets"], b["dets"]))
        t_y, t_c, t_r = [], [], []
        for _ in range(REPS):
            t_y.append(clock(lambda: dets(yuyv, "yuyv")))
            t_c.append(clock(convert))
            t_r.append(clock(lambda: dets(rgb, None)))
        t_both = [c + r for c, r in zip(t_c, t_r)]
        print(f"  {w}x{h}, {n} frames per call (chunks of {B}):")
        print(f"    YUYV bytes -> records (pix entry):            {fmt_rate(n, t_y)}  [layer 0 {l0}]")
        print(f"    host conversion, {THREADS} threads, then RGB entry:  {fmt_rate(n, t_both)}  [conversion {spread(t_c)[0] / CHUNKS * 1e3:.2f} ms per chunk; "
              f"RGB entry alone {fmt_rate(n, t_r)}]")
        print(f"    YUYV / (convert + RGB) = {spread(t_both)[0] / spread(t_y)[0]:.3f}x the rate; YUYV / RGB entry alone = {spread(t_r)[0] / spread(t_y)[0]:.3f}x")
        for name, imgs in (("YUYV", yuyv), ("RGB ", rgb)):
            t_stage, t_h2d, nbytes = chunk_stages(imgs, B)
            t_call = spread(t_y if name == "YUYV" else t_r)[0]
            print(f"    per chunk {name}: staging copy {t_stage * 1e3:.2f} ms ({B * nbytes / t_stage / 1e9:.1f} GB/s, {THREADS} threads), "
                  f"H2D {t_h2d * 1e3:.2f} ms ({B * nbytes / t_h2d / 1e9:.1f} GB/s), GPU (network only) {t_net * 1e3:.2f} ms; call / chunk {t_call / CHUNKS * 1e3:.2f} ms")
        del rgb, yuyv
ctx.close()
