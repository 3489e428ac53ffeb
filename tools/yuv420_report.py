#!/usr/bin/env python3
"""Rate of NV12 / I420 video frames -> detection records (GPU box): the _pix_dets entries reading planar YUV 4:2:0 bytes on the GPU
(yolo2_hip_run_images_pix_dets[_f16] with YOLO2_PIX_NV12 / YOLO2_PIX_I420) beside the same entries on the same pictures as packed
YUYV and as RGB24, i.e. 1.5, 1.5, 2 and 3 bytes per pixel through staging and H2D.  768x576 frames from tests/golden/dog.npz, fp16 at
batch 256 and int16 at batch 64, one process; after a warm-up call the four formats alternate and every figure is the median of the
repeats with their spread (min .. max); every timed window ends in a device synchronise.  Per chunk it also prices the stages the
entries overlap - staging copy (pageable -> pinned, four threads), H2D of the chunk's bytes, GPU (network only) - and, for the fp16
pass, the device-event time of the layer-0 kernel of each format (yolo2_hip_layer_times_ms, slot 0).
usage: python3 tools/yuv420_report.py [chunks per call = 8] [reps = 3]
The layer-0 kernels alone, from a trace (no counters):
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o l0 -- python3 tools/yuv420_report.py --trace
  python3 tools/yuv420_report.py --summary <dir>/.../l0_kernel_stats.csv"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import yuv420ref
from yolo2_amd import hipdrv, synth

TRACE_CALLS, TRACE_B = 8, 256
if len(sys.argv) > 2 and sys.argv[1] == "--summary":      # the trace's kernel statistics: summed time of each format's layer-0 kernel per frame
    import csv
    rows = {r["Name"]: r for r in csv.DictReader(open(sys.argv[2]))}
    print(f"# layer-0 kernels, {TRACE_CALLS} calls of {TRACE_B} frames per format, alternating: rocprofv3 --kernel-trace --stats, summed kernel time per frame "
          "(fastest .. slowest launch, a launch is one lane's share of a chunk)")
    per_frame = {}
    for f in ("nv12", "i420", "yuyv", "u8"):
        hits = [r for n, r in rows.items() if f"k_conv0_pool_mfma_{f}ILb0E" in n or n.startswith(f"void y2::k_conv0_pool_mfma_{f}<false>")]
        assert len(hits) == 1, (f, list(rows))
        calls, total, lo, hi = int(hits[0]["Calls"]), float(hits[0]["TotalDurationNs"]) / 1e3, float(hits[0]["MinNs"]) / 1e3, float(hits[0]["MaxNs"]) / 1e3
        share = TRACE_CALLS * TRACE_B / calls
        per_frame[f] = total / (TRACE_CALLS * TRACE_B)
        print(f"k_conv0_pool_mfma_{f:4s} {calls:3d} launches {total / 1e3:8.3f} ms = {per_frame[f]:5.2f} us/frame ({lo / share:5.2f} .. {hi / share:5.2f})")
    print(f"nv12 / yuyv = {per_frame['nv12'] / per_frame['yuyv']:.3f}, i420 / yuyv = {per_frame['i420'] / per_frame['yuyv']:.3f}, "
          f"nv12 / u8 = {per_frame['nv12'] / per_frame['u8']:.3f}, i420 / u8 = {per_frame['i420'] / per_frame['u8']:.3f}")
    sys.exit(0)
TRACE = len(sys.argv) > 1 and sys.argv[1] == "--trace"
if TRACE:
    del sys.argv[1]
CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
THREADS = 4     # kStageThreads of the entries' staging copy
FORMATS = ("nv12", "i420", "yuyv", "rgb24")
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
pool = ThreadPoolExecutor(THREADS)
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576


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
    t_stage = spread([clock(lambda: list(pool.map(part, range(THREADS)))) for _ in range(5)])[0]
    dbuf = torch.empty(B * nbytes, dtype=torch.uint8, device=dev)
    dbuf.copy_(pinned, non_blocking=True)
    torch.cuda.synchronize()
    t_h2d = spread([clock(lambda: dbuf.copy_(pinned, non_blocking=True)) for _ in range(8)])[0]
    return t_stage, t_h2d, nbytes


# 16 pictures (the dog picture shifted sideways), each in the four formats: the NV12 frame is the source, the others hold the same
# picture - I420 the same planes, YUYV and RGB24 its conversion - so the records of all four are the same
base = {f: [] for f in FORMATS}
for k in range(16):
    nv12 = yuv420ref.from_rgb(np.roll(DOG, 48 * k, axis=1), "nv12")
    base["nv12"].append(nv12)
    base["i420"].append(yuv420ref.pack(*yuv420ref.planes(nv12, "nv12"), "i420"))
    base["yuyv"].append(yuv420ref.to_yuyv(nv12, "nv12"))
    base["rgb24"].append(yuv420ref.to_rgb(nv12, "nv12"))
h, w = DOG.shape[:2]

if TRACE:      # what the trace is taken of: the fp16 pass from one chunk of each format, alternating
    ctx.run_images_f16_host(base["rgb24"][:2], 2, pixfmt="rgb24")
    for _ in range(TRACE_CALLS):
        for f in FORMATS:
            ctx.run_images_f16_host([base[f][i % 16] for i in range(TRACE_B)], TRACE_B, pixfmt=f)
    ctx.close()
    sys.exit(0)

print(f"# python3 tools/yuv420_report.py {CHUNKS} {REPS}   (one process, one MI355X; synthetic weights SynthModel(seed=1), {w}x{h} frames from "
      f"tests/golden/dog.npz; a warm-up call per format, then median of {REPS} alternating repeats (min .. max))")
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
    n = CHUNKS * B
    imgs = {f: [base[f][i % 16] for i in range(n)] for f in FORMATS}
    dets = lambda f: hipdrv.run_images_dets(ctx._h, imgs[f], B, 0.25, 0.45, cap=100, precision=precision, pixfmt=f)
    l0, ref = {}, None
    for f in FORMATS:                                   # untimed: buffers, plans; and the records agree
        r = dets(f)
        if precision == "fp16":
            l0[f] = ctx.images_layer0_kernel(False)
        else:
            l0[f] = {"nv12": "k_letterbox_nv12_batch", "i420": "k_letterbox_i420_batch", "yuyv": "k_letterbox_yuyv_batch",
                     "rgb24": "k_letterbox_u8_batch"}[f] + " + the int16 table"
        if ref is None:
            ref = r
        assert np.array_equal(r["counts"], ref["counts"]) and all(x.tobytes() == y.tobytes() for x, y in zip(r["dets"], ref["dets"])), f
    times = {f: [] for f in FORMATS}
    for _ in range(REPS):
        for f in FORMATS:
            times[f].append(clock(lambda: dets(f)))
    print(f"  {w}x{h}, {n} frames per call (chunks of {B}), bytes -> records (pix entry); the records of the four formats are identical:")
    for f in FORMATS:
        print(f"    {f.upper():5s} {imgs[f][0].nbytes / (w * h):.1f} B/px: {fmt_rate(n, times[f])}  [layer 0 {l0[f]}]")
    med = {f: spread(times[f])[0] for f in FORMATS}
    lo_rgb, hi_rgb = n / spread(times["rgb24"])[2], n / spread(times["rgb24"])[1]
    for f in ("nv12", "i420"):
        print(f"    {f.upper()} / RGB24 = {med['rgb24'] / med[f]:.3f}x the rate, {f.upper()} / YUYV = {med['yuyv'] / med[f]:.3f}x"
              f"   (RGB24's repeats spread over {hi_rgb - lo_rgb:.0f} frames/s: {n / med[f]:.0f} >= {n / med['rgb24']:.0f} - {hi_rgb - lo_rgb:.0f} is "
              f"{n / med[f] >= n / med['rgb24'] - (hi_rgb - lo_rgb)})")
    for f in FORMATS:
        t_stage, t_h2d, nbytes = chunk_stages(imgs[f], B)
        print(f"    per chunk {f.upper():5s}: staging copy {t_stage * 1e3:.2f} ms ({B * nbytes / t_stage / 1e9:.1f} GB/s, {THREADS} threads), "
              f"H2D {t_h2d * 1e3:.2f} ms ({B * nbytes / t_h2d / 1e9:.1f} GB/s), GPU (network only) {t_net * 1e3:.2f} ms; call / chunk {med[f] / CHUNKS * 1e3:.2f} ms")
    if precision == "fp16":
        # device events around the layer-0 launch of lane 0 (its share of the chunk's 256 frames; the other lane's launches run beside it), one chunk per
        # call, 8 calls per format, the formats alternating
        ev = {f: [] for f in FORMATS}
        one = {f: imgs[f][:B] for f in FORMATS}
        for _ in range(8):
            for f in FORMATS:
                ctx.set_profiling(True)
                ctx.run_images_f16_host(one[f], B, pixfmt=f)
                ev[f].append(float(ctx.layer_times_ms()[0]))
        ctx.set_profiling(False)
        per = B // max(1, ctx.num_lanes_fp16())
        print(f"    layer-0 kernel, device-event time of lane 0's launch ({per} frames), median of 8 (min .. max):")
        for f in FORMATS:
            m, lo, hi = spread(ev[f])
            print(f"      {l0[f]:28s} {m * 1e3:7.1f} us = {m * 1e3 / per:5.2f} us/frame ({lo * 1e3:.1f} .. {hi * 1e3:.1f})"
                  + (f"   = {m / spread(ev['yuyv'])[0]:.3f} of the YUYV kernel's" if f in ("nv12", "i420") else ""))
    del imgs
ctx.close()
