#!/usr/bin/env python3
"""Rate of the camera loop as one call (GPU box): yolo2_hip_loop_images_pix (JPEG out and RGB24 out) against the two-call route it
joins - the _pix_dets entry of the precision, then the matching annotate entry fed those records (the frame bytes staged and
uploaded twice, the records round-tripped, the draw items made on the host) - in the same process.  Input: the dog frame of
tests/golden/dog.npz rolled by a different offset per frame, 768x576, as YUYV and as RGB24; SynthModel(seed=1, obj_bias=2.0);
thresh 0.24; quality 80.  Passes: int16 at batch 64, fp16 at batch 256.  At 0.24 this model leaves no record on these frames (the
painter then only converts), so every row is measured a second time at thresh 0.1, where k_draw_items and the painter have records.
The routes alternate; every figure is the median of the repeats with their spread (min .. max).  Also: the frame bytes each route
uploads.
usage: python3 tools/loop_report.py [chunks per call = 4] [reps = 5] [tree]
       python3 tools/loop_report.py --trace     (two loop calls at int16 / batch 64 / YUYV / JPEG / thresh 0.1, where the frames have records, for
                                                 rocprofv3 --kernel-trace --stats -- python3 tools/loop_report.py --trace: k_draw_items' time)"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
from yolo2_amd import hipdrv, synth

TRACE = len(sys.argv) > 1 and sys.argv[1] == "--trace"
CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 and not TRACE else 4
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
TREE = sys.argv[3] if len(sys.argv) > 3 else ""
QUALITY, THRESH, NMS, CAP = 80, 0.24, 0.45, 845
THRESHES = (THRESH, 0.1)
W, H = 768, 576
NAMES = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def clock(fn):      # (every entry is synchronous)
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt_rate(n, ts):
    med, lo, hi = spread(ts)
    return f"{med * 1e3:.1f} ms per call = {n / med:.0f} frames/s ({n / hi:.0f} .. {n / lo:.0f})"


def to_yuyv(rgb):
    """BT.601 studio-range YUYV of an RGB frame (the report's camera frames; the entries convert them back on the GPU)"""
    r, g, b = (rgb[:, :, k].astype(np.float32) for k in range(3))
    y = np.clip(np.rint(16 + .257 * r + .504 * g + .098 * b), 0, 255)
    u = np.clip(np.rint(128 - .148 * r - .291 * g + .439 * b), 0, 255)
    v = np.clip(np.rint(128 + .439 * r - .368 * g - .071 * b), 0, 255)
    out = np.empty((rgb.shape[0], rgb.shape[1], 2), dtype=np.uint8)
    out[:, :, 0] = y
    out[:, 0::2, 1] = u[:, 0::2]
    out[:, 1::2, 1] = v[:, 0::2]
    return out


def tree():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD^{tree}"], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
        return head + (" + uncommitted changes" if dirty else "") if head else "unknown"
    except OSError:
        return "unknown"


model = synth.SynthModel(seed=1, obj_bias=2.0)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
base_rgb = [np.ascontiguousarray(np.roll(DOG, (37 * i, 53 * i), axis=(0, 1))) for i in range(16)]
base_yuyv = [to_yuyv(im) for im in base_rgb]

if TRACE:
    imgs = [base_yuyv[i % 16] for i in range(128)]
    for _ in range(2):
        ctx.loop_images(imgs, pixfmt="yuyv", precision="int16", thresh=THRESHES[1], nms=NMS, labels=NAMES, jpeg_quality=QUALITY, batch=64, cap=CAP)
    ctx.close()
    sys.exit(0)

ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
print(f"# python3 tools/loop_report.py {CHUNKS} {REPS}{' ' + TREE if TREE else ''}   (one process, one MI355X; {W}x{H} dog frames rolled per frame, SynthModel(seed=1, obj_bias=2.0), "
      f"thresh {' and '.join(str(t) for t in THRESHES)}, quality {QUALITY}; median of {REPS} alternating repeats (min .. max); tree {TREE or tree()})")
pad = lambda b: (b + 255) & ~255
for precision, B in (("int16", 64), ("fp16", 256)):
    n = CHUNKS * B
    for pixfmt, base in (("yuyv", base_yuyv), ("rgb24", base_rgb)):
        imgs = [base[i % 16] for i in range(n)]
        frame_bytes = sum(pad(im.nbytes) for im in imgs)
        for out, quality, thresh in [(o, q, t) for t in THRESHES for o, q in (("JPEG", QUALITY), ("RGB24", None))]:
            loop = lambda: ctx.loop_images(imgs, pixfmt=pixfmt, precision=precision, thresh=thresh, nms=NMS, labels=NAMES, jpeg_quality=quality,
                                           batch=B, cap=CAP)

            def two():
                r = hipdrv.run_images_dets(ctx._h, imgs, B, thresh, NMS, cap=CAP, precision=precision, pixfmt=pixfmt)
                return r, ctx.annotate_images(imgs, r["dets"], None, B, thresh, labels=NAMES, pixfmt=pixfmt, jpeg_quality=quality)
            got = loop()      # untimed: buffers, plans
            info = ctx.loop_last_info()
            r, (frames, drawn) = two()
            same = all(np.array_equal(a, b) if quality is None else a == b for a, b in zip(got["frames"], frames)) and \
                all(a.tobytes() == b.tobytes() for a, b in zip(got["dets"], r["dets"]))
            t_l, t_t = [], []
            for _ in range(REPS):
                t_l.append(clock(loop))
                t_t.append(clock(two))
            print(f"{precision}, batch {B}, {pixfmt} in, {out} out, thresh {thresh}, {n} frames per call, {np.mean(drawn):.1f} records drawn per frame, outputs "
                  f"{'identical' if same else 'DIFFER'}:")
            print(f"    loop entry (one call):                      {fmt_rate(n, t_l)}")
            print(f"    _pix_dets, then annotate (two calls):       {fmt_rate(n, t_t)}  -> loop / two calls = {spread(t_t)[0] / spread(t_l)[0]:.2f}x")
            print(f"    frame bytes uploaded: loop {info['image_bytes_h2d'] / 1e6:.1f} MB in {info['chunks']} chunks (tables included), two calls "
                  f"{2 * frame_bytes / 1e6:.1f} MB (the padded frames, twice); loop D2H of frames / streams {info['out_bytes_d2h'] / 1e6:.1f} MB; "
                  f"{info['items_built']} items from {info['items_kernel']}")
            del got, frames
        del imgs
ctx.close()
