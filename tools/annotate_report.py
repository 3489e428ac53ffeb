#!/usr/bin/env python3
"""Rate of annotated frames (GPU box): yolo2_hip_annotate_images_pix_host at 768x576 from YUYV and RGB24 frames, batches 64 and 256,
against (a) a bare pinned device-to-host copy of the same output bytes - the ceiling the entry can approach, since every annotated
frame crosses PCIe back as 3 bytes per pixel -, (b) the route the CLI's writer takes without --annotate-gpu, on four host threads:
y2h::plain_box_frame - y2h::yuyv_to_rgb24 + every pixel into a float image + y2h::draw_box per record, the function the CLI calls; no
labels, no PPM -, and (c) the _dets entry alone and _dets followed by annotate on the same frames (the image bytes cross PCIe twice).
One process; the routes alternate; every figure is the median of the repeats with their spread (min .. max).
usage: python3 tools/annotate_report.py [chunks per call = 4] [reps = 5] [tree = `git rev-parse HEAD^{tree}` of this checkout]
tree: the hash the report names as the tree it was taken on, for a copy of the sources without git metadata."""
import ctypes as C
import os, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, synth

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
TREE = sys.argv[3] if len(sys.argv) > 3 else ""
THREADS = 4
W, H = 768, 576
THRESH, NMS = 0.25, 0.45
dev = torch.device("cuda:0")
host = C.CDLL(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "libyolo2_host.so"))
host.y2h_plain_box_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
host.y2h_plain_box_frame.restype = C.c_double
NAMES = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
model = synth.SynthModel(seed=1, obj_bias=2.0)
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


def upload_time(imgs):
    """pinned H2D of these images' bytes, alone, median seconds"""
    nbytes = sum(im.nbytes for im in imgs)
    pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dbuf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    clock(lambda: dbuf.copy_(pinned, non_blocking=True))
    return spread([clock(lambda: dbuf.copy_(pinned, non_blocking=True)) for _ in range(8)])[0]


def tree():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD^{tree}"], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
        return head + (" + uncommitted changes" if dirty else "") if head else "unknown"
    except OSError:
        return "unknown"


print(f"# python3 tools/annotate_report.py {CHUNKS} {REPS}   (one process, one MI355X; {W}x{H} random-byte frames, records of SynthModel(seed=1, obj_bias=2.0) "
      f"at thresh {THRESH}; median of {REPS} alternating repeats (min .. max); tree {TREE or tree()})")
base_yuyv = [rng.integers(0, 256, (H, W, 2), dtype=np.uint8) for _ in range(16)]
base_rgb = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(16)]
for precision, B in (("int16", 64), ("fp16", 256)):
    n = CHUNKS * B
    out_bytes = B * W * H * 3
    pinned = torch.empty(out_bytes, dtype=torch.uint8).pin_memory()
    dbuf = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    clock(lambda: pinned.copy_(dbuf, non_blocking=True))
    t_d2h = spread([clock(lambda: pinned.copy_(dbuf, non_blocking=True)) for _ in range(8)])[0]
    print(f"batch {B} ({precision} records): bare pinned D2H of one chunk's output ({out_bytes / 1e6:.0f} MB): {t_d2h * 1e3:.2f} ms = {out_bytes / t_d2h / 1e9:.1f} GB/s "
          f"= {B / t_d2h:.0f} frames/s")
    del pinned, dbuf
    for pixfmt, base in (("yuyv", base_yuyv), ("rgb24", base_rgb)):
        imgs = [base[i % 16] for i in range(n)]
        dets = lambda: hipdrv.run_images_dets(ctx._h, imgs, B, THRESH, NMS, cap=845, precision=precision, pixfmt=pixfmt)
        r = dets()
        packed = np.zeros((n, 845), dtype=hipdrv.DET_DTYPE)
        for f, d in enumerate(r["dets"]):
            packed[f, :len(d)] = d
        counts = r["counts"]
        anno = lambda: ctx.annotate_images(imgs, packed, counts, B, THRESH, labels=NAMES, pixfmt=pixfmt)
        outs, drawn = anno()                # untimed: buffers

        def host_route():
            def part(t):
                for i in range(t, n, THREADS):
                    m = min(int(counts[i]), 845)
                    host.y2h_plain_box_frame(imgs[i].ctypes.data, W, H, int(pixfmt == "yuyv"), packed[i].ctypes.data, m, 80)
            list(pool.map(part, range(THREADS)))
        t_a, t_h, t_d, t_da = [], [], [], []
        for _ in range(REPS):
            t_a.append(clock(anno))
            t_h.append(clock(host_route))
            t_d.append(clock(dets))
            t_da.append(clock(lambda: (dets(), anno())))
        a = spread(t_a)[0]
        print(f"  {pixfmt}, {n} frames per call (chunks of {B}), {drawn.mean():.1f} records drawn per frame:")
        print(f"    annotate entry (bytes -> annotated RGB24 on the host):   {fmt_rate(n, t_a)}  = {n / a / (B / t_d2h):.2f} of the bare D2H ceiling")
        print(f"    host route, {THREADS} threads (convert + float image + draw_box): {fmt_rate(n, t_h)}  -> entry / host route = {spread(t_h)[0] / a:.1f}x")
        print(f"    _dets entry alone:                                        {fmt_rate(n, t_d)}")
        print(f"    _dets, then annotate (bytes uploaded twice):              {fmt_rate(n, t_da)}  = {spread(t_d)[0] / spread(t_da)[0]:.2f} of the _dets rate")
        t_up = upload_time(imgs[:B])
        print(f"    the second upload: pinned H2D of one chunk's image bytes {t_up * 1e3:.2f} ms = {t_up / (a / CHUNKS):.2f} of the annotate entry's time per chunk "
              f"(D2H of its output: {t_d2h / (a / CHUNKS):.2f})")
        del imgs, outs, packed
ctx.close()
