#!/usr/bin/env python3
"""Rate of the camera loop with the annotated frames back as planar YUV 4:2:0 (GPU box): yolo2_hip_loop_images_pix with
YOLO2_LOOP_OUT_NV12 / _I420 beside YOLO2_LOOP_OUT_RGB24, and beside the route a caller who feeds a video encoder had before: RGB24 out
followed by the conversion on host threads (y2h_rgb24_to_yuv420, libyolo2_host.so's plain loop, on 4 and on 16 threads).  768x576 NV12
frames in (a decoder's own format) made from tests/golden/dog.npz; fp16 at batch 256, int16 at batch 64; one process; after a warm-up
call per variant the variants alternate and every figure is the median of the repeats with their spread (min .. max); every timed
window ends in a device synchronise.  Also: the bytes that come back per frame (yolo2_hip_loop_last_info).
usage: python3 tools/yuvout_report.py [chunks per call = 2] [reps = 3] [--stats DIR]
       python3 tools/yuvout_report.py --trace
--trace: a short run for a profiler - rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/yuvout_report.py --trace - with the same
number of chunks (4, of 256 frames, fp16) through each of the three painters; --stats DIR then adds the painters' rows of the
kernel statistics found under DIR to the report (device time per launch = per chunk)."""
import csv, glob, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import yuv420ref
from yolo2_amd import hipdrv, synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
TRACE = "--trace" in sys.argv
STATS = sys.argv[sys.argv.index("--stats") + 1] if "--stats" in sys.argv else None
if STATS in args:
    args.remove(STATS)
CHUNKS = int(args[0]) if len(args) > 0 else 2
REPS = int(args[1]) if len(args) > 1 else 3
ORDERS = ("rgb", "nv12", "i420")
KERNEL = {"rgb": "k_annotate_batch", "nv12": "k_annotate_batch_nv12", "i420": "k_annotate_batch_i420"}
model = synth.SynthModel(seed=1, obj_bias=2.0)       # (obj_bias: records exist, so boxes and tags are painted)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
pools = {t: ThreadPoolExecutor(t) for t in (4, 16)}
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
H = hipdrv.host_lib()
NAMES = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
h, w = DOG.shape[:2]
base = [yuv420ref.from_rgb(np.ascontiguousarray(np.roll(DOG, 48 * k, axis=1)), "nv12") for k in range(16)]


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


def convert(frames, threads, outs):
    """the host pass: every RGB24 frame through y2h_rgb24_to_yuv420 (ctypes releases the GIL) into its preallocated NV12 array"""
    def part(t):
        for i in range(t, len(frames), threads):
            H.y2h_rgb24_to_yuv420(frames[i].ctypes.data, w, h, 1, outs[i].ctypes.data)
    list(pools[threads].map(part, range(threads)))
    return outs


def loop(imgs, precision, B, order):
    return ctx.loop_images(imgs, pixfmt="nv12", precision=precision, thresh=0.07, nms=0.45, labels=NAMES, batch=B, cap=100, out_order=order)


if TRACE:
    imgs = [base[i % 16] for i in range(4 * 256)]
    for order in ORDERS:
        r = loop(imgs, "fp16", 256, order)
        print(f"{KERNEL[order]}: 4 chunks of 256 frames, {int(r['drawn'].sum())} records drawn")
    ctx.close()
    sys.exit(0)

print(f"# python3 tools/yuvout_report.py {CHUNKS} {REPS}   (one process, one MI355X; synthetic weights SynthModel(seed=1, obj_bias=2.0), {w}x{h} NV12 "
      f"frames in, made from tests/golden/dog.npz; a warm-up call per variant, then median of {REPS} alternating repeats (min .. max))")
for precision, B in (("fp16", 256), ("int16", 64)):
    n = CHUNKS * B
    imgs = [base[i % 16] for i in range(n)]
    back, want = {}, None
    for order in ORDERS:                                   # untimed: buffers, plans; the 4:2:0 frames are the RGB24 frames converted
        r = loop(imgs, precision, B, order)
        back[order] = ctx.loop_last_info()["out_bytes_d2h"] / n
        if order == "rgb":
            want, drawn = r["frames"][:16], int(r["drawn"].sum())
        else:
            assert all(np.array_equal(a, hipdrv.rgb24_to_yuv420(b, order)) for a, b in zip(r["frames"][:16], want)), order
        del r
    scratch = [np.empty((h * 3 // 2, w), dtype=np.uint8) for _ in range(n)]      # the host route's NV12 frames, written anew by every call
    host = lambda t: convert(loop(imgs, precision, B, "rgb")["frames"], t, scratch)
    times = {o: [] for o in ORDERS}
    host_times, convert_times = {4: [], 16: []}, {4: [], 16: []}
    rgb_frames = loop(imgs, precision, B, "rgb")["frames"]
    for _ in range(REPS):
        for o in ORDERS:
            times[o].append(clock(lambda: loop(imgs, precision, B, o)))
        for t in host_times:
            host_times[t].append(clock(lambda: host(t)))
            convert_times[t].append(clock(lambda: convert(rgb_frames, t, scratch)))
    print(f"{precision}, {n} frames per call in chunks of {B}, records + annotated frames back ({drawn} records drawn per call); "
          f"the NV12 / I420 frames are y2h_rgb24_to_yuv420 of the RGB24 frames:")
    med = {o: spread(times[o])[0] for o in ORDERS}
    lo_rgb, hi_rgb = n / spread(times["rgb"])[2], n / spread(times["rgb"])[1]
    for o in ORDERS:
        note = "" if o == "rgb" else f"   = {med['rgb'] / med[o]:.3f}x the RGB24-out rate (whose repeats spread over {hi_rgb - lo_rgb:.0f} frames/s)"
        print(f"    {o.upper() + ('24' if o == 'rgb' else ''):5s} out ({KERNEL[o]}), {back[o] / 1e3:.1f} kB back per frame: {fmt_rate(n, times[o])}{note}")
    print("  the route without the formats: RGB24 out, then y2h_rgb24_to_yuv420 on host threads (a plain C++ loop, pageable -> pageable):")
    for t, ts in host_times.items():
        m, cm = spread(ts)[0], spread(convert_times[t])[0]
        print(f"    RGB24 out + conversion on {t:2d} threads: {fmt_rate(n, ts)}; the conversion alone {cm * 1e3:.1f} ms = {n / cm:.0f} frames/s; "
              f"NV12 out is {m / med['nv12']:.3f}x, I420 out {m / med['i420']:.3f}x this route's rate")
    del scratch, rgb_frames, imgs, want
ctx.close()

if STATS:
    rows = []
    for path in glob.glob(os.path.join(STATS, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if r.get("Name", "").split("(")[0].split("::")[-1].strip() in KERNEL.values()]
    print("the painters alone, device time per launch = per chunk of 256 frames (fp16, 4 chunks per painter; rocprofv3 --kernel-trace --stats of "
          "`tools/yuvout_report.py --trace`, a run of its own):")
    name = lambda r: r["Name"].split("(")[0].split("::")[-1].strip()
    avg = lambda r: float(r["TotalDurationNs"]) / max(1, int(r["Calls"]))
    t_rgb = next((avg(r) for r in rows if name(r) == "k_annotate_batch"), None)
    for r in sorted(rows, key=name):
        lo_hi = f" ({float(r['MinNs']) / 1e3:.1f} .. {float(r['MaxNs']) / 1e3:.1f})" if "MinNs" in r and "MaxNs" in r else ""
        print(f"    {name(r):24s} {r['Calls']} launches, average {avg(r) / 1e3:.1f} us{lo_hi} = {avg(r) / 1e3 / 256:.2f} us/frame"
              + (f" = {avg(r) / t_rgb:.3f} of k_annotate_batch's" if t_rgb else ""))
    if not rows:
        print("    (no kernel statistics found under " + STATS + ")")
