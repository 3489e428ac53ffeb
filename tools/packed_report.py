#!/usr/bin/env python3
"""Rate of packed BGR24 / RGBA32 / BGRA32 frames -> detection records (GPU box): the _pix_dets entries reading the frames as the caller
holds them (YOLO2_PIX_BGR24 / _RGBA32 / _BGRA32, the bytes picked where the GPU fetches a pixel) beside the same pictures as RGB24,
and beside the route such a caller had before: the byte reorder on host threads (y2h_packed_to_rgb24, libyolo2_host.so's plain loop,
on 4 and on 16 threads) followed by the RGB24 entry.  768x576 frames from tests/golden/dog.npz; fp16 at batch 256, int16 at batch 64,
int8 at batch 256; one process; after a warm-up call the formats alternate and every figure is the median of the repeats with their
spread (min .. max); every timed window ends in a device synchronise.  Per chunk it also prices the stages the entries overlap -
staging copy (pageable -> pinned, four threads), H2D of the chunk's bytes, GPU (network only) - and, for the fp16 pass, the
device-event time of each format's layer-0 kernel (yolo2_hip_layer_times_ms, slot 0) and the camera loop with RGB24 and BGR24 output.
usage: python3 tools/packed_report.py [chunks per call = 8] [reps = 3]"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import packedref
from yolo2_amd import hipdrv, synth

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
THREADS = 4     # kStageThreads of the entries' staging copy
FORMATS = ("bgr24", "rgba32", "bgra32", "rgb24")
PACKED = FORMATS[:3]
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
ctx8 = hipdrv.Yolo2Hip(0)
ctx8.load_weights_fp32(model.weights_f32(), model.bias_f32())
ctx8.load_model(ctx8.calibrate_int8(frames=synth.frames(40, 4), batch=4))
pools = {t: ThreadPoolExecutor(t) for t in (4, 16)}
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
H = hipdrv.host_lib()


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


def reorder(imgs, f, threads, outs):
    """the host pass: every frame through y2h_packed_to_rgb24 (ctypes releases the GIL) into its preallocated RGB24 array"""
    code = hipdrv.PIXFMTS_PACKED[f]
    def part(t):
        for i in range(t, len(imgs), threads):
            H.y2h_packed_to_rgb24(imgs[i].ctypes.data, imgs[i].shape[1], imgs[i].shape[0], code, outs[i].ctypes.data)
    list(pools[threads].map(part, range(threads)))
    return outs


def chunk_stages(imgs, B):
    """(staging copy, H2D) seconds of one chunk of B frames, each alone, medians"""
    nbytes = imgs[0].nbytes
    pinned = torch.empty(B * nbytes, dtype=torch.uint8).pin_memory()
    view = pinned.numpy()
    def part(t):
        for i in range(t, B, THREADS):
            view[i * nbytes:(i + 1) * nbytes] = imgs[i].reshape(-1)
    t_stage = spread([clock(lambda: list(pools[4].map(part, range(THREADS)))) for _ in range(5)])[0]
    dbuf = torch.empty(B * nbytes, dtype=torch.uint8, device=dev)
    dbuf.copy_(pinned, non_blocking=True)
    torch.cuda.synchronize()
    t_h2d = spread([clock(lambda: dbuf.copy_(pinned, non_blocking=True)) for _ in range(8)])[0]
    return t_stage, t_h2d, nbytes


# 16 pictures (the dog picture shifted sideways), each in the four formats: the records of all four are the same
base = {f: [] for f in FORMATS}
rng = np.random.default_rng(1)
for k in range(16):
    rgb = np.ascontiguousarray(np.roll(DOG, 48 * k, axis=1))
    base["rgb24"].append(rgb)
    for f in PACKED:
        base[f].append(packedref.from_rgb(rgb, f, rng.integers(0, 256, rgb.shape[:2], dtype=np.uint8)))
h, w = DOG.shape[:2]
LB = {"bgr24": "k_letterbox_bgr24_batch", "rgba32": "k_letterbox_rgba32_batch", "bgra32": "k_letterbox_bgra32_batch", "rgb24": "k_letterbox_u8_batch"}

print(f"# python3 tools/packed_report.py {CHUNKS} {REPS}   (one process, one MI355X; synthetic weights SynthModel(seed=1), {w}x{h} frames from "
      f"tests/golden/dog.npz; a warm-up call per format, then median of {REPS} alternating repeats (min .. max))")
for precision, B in (("fp16", 256), ("int16", 64), ("int8", 256)):
    c = ctx8 if precision == "int8" else ctx
    frames = torch.from_numpy(synth.frames(7, B)).to(dev)
    if precision == "int16":
        c.set_batch(B)
        region = torch.empty((B, 425, 13, 13), dtype=torch.int16, device=dev)
        net = lambda: c.run_batch_ptr(frames.data_ptr(), B, region.data_ptr(), st)
    else:
        region = torch.empty((B, 425, 13, 13), dtype=torch.float32, device=dev)
        if precision == "fp16":
            net = lambda: c.run_batch_fp16_ptr(frames.data_ptr(), B, region.data_ptr(), st)
        else:
            net = lambda: c.run_batch_int8_ptr(frames.data_ptr(), B, region.data_ptr(), st)
    clock(net)
    t_net = spread([clock(net) for _ in range(8)])[0]
    print(f"{precision} batch {B}: network only (letterboxed fp32 frames resident in HBM): {t_net * 1e3:.2f} ms per chunk = {B / t_net:.0f} frames/s")
    del frames, region
    n = CHUNKS * B
    imgs = {f: [base[f][i % 16] for i in range(n)] for f in FORMATS}
    dets = lambda f, ims=None: hipdrv.run_images_dets(c._h, imgs[f] if ims is None else ims, B, 0.25, 0.45, cap=100, precision=precision, pixfmt=f)
    l0, ref = {}, None
    for f in FORMATS[::-1]:                                   # untimed: buffers, plans; and the records agree
        r = dets(f)
        l0[f] = c.images_layer0_kernel(False) if precision == "fp16" else c.images_front_kernel_int8() if precision == "int8" else LB[f] + " + the int16 table"
        if ref is None:
            ref = r
        assert np.array_equal(r["counts"], ref["counts"]) and all(x.tobytes() == y.tobytes() for x, y in zip(r["dets"], ref["dets"])), f
    scratch = [np.empty((h, w, 3), dtype=np.uint8) for _ in range(n)]      # the host route's RGB24 frames, written anew by every call
    host = lambda f, t: dets("rgb24", reorder(imgs[f], f, t, scratch))
    times = {f: [] for f in FORMATS}
    host_times = {(f, t): [] for f in ("bgr24", "bgra32") for t in (4, 16)}
    reorder_times = {k: [] for k in host_times}
    for _ in range(REPS):
        for f in FORMATS:
            times[f].append(clock(lambda: dets(f)))
        for key in host_times:
            host_times[key].append(clock(lambda: host(*key)))
            reorder_times[key].append(clock(lambda: reorder(imgs[key[0]], key[0], key[1], scratch)))
    print(f"  {w}x{h}, {n} frames per call (chunks of {B}), bytes -> records (pix entry); the records of the four formats are identical:")
    for f in FORMATS:
        print(f"    {f.upper():6s} {imgs[f][0].nbytes / (w * h):.1f} B/px: {fmt_rate(n, times[f])}  [layer 0 {l0[f]}]")
    med = {f: spread(times[f])[0] for f in FORMATS}
    lo_rgb, hi_rgb = n / spread(times["rgb24"])[2], n / spread(times["rgb24"])[1]
    for f in PACKED:
        print(f"    {f.upper()} / RGB24 = {med['rgb24'] / med[f]:.3f}x the rate   (RGB24's repeats spread over {hi_rgb - lo_rgb:.0f} frames/s)")
    print("  the route without the formats: y2h_packed_to_rgb24 on host threads (a plain C++ loop, pageable -> pageable), then the RGB24 entry:")
    for (f, t), ts in host_times.items():
        m = spread(ts)[0]
        rm = spread(reorder_times[(f, t)])[0]
        rd = imgs[f][0].nbytes + w * h * 3
        print(f"    {f.upper():6s} reorder on {t:2d} threads + RGB24 entry: {fmt_rate(n, ts)}; the reorder alone {rm * 1e3:.1f} ms = {n / rm:.0f} frames/s "
              f"({n * rd / rm / 1e9:.1f} GB/s read + written); the {f.upper()} entry is {m / med[f]:.3f}x this route's rate")
    for f in FORMATS:
        t_stage, t_h2d, nbytes = chunk_stages(imgs[f], B)
        print(f"    per chunk {f.upper():6s}: staging copy {t_stage * 1e3:.2f} ms ({B * nbytes / t_stage / 1e9:.1f} GB/s, {THREADS} threads), "
              f"H2D {t_h2d * 1e3:.2f} ms ({B * nbytes / t_h2d / 1e9:.1f} GB/s), GPU (network only) {t_net * 1e3:.2f} ms; call / chunk {med[f] / CHUNKS * 1e3:.2f} ms")
    del scratch
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
        u8 = spread(ev["rgb24"])
        for f in FORMATS:
            m, lo, hi = spread(ev[f])
            note = "" if f == "rgb24" else f"   = {m / u8[0]:.3f} of the RGB24 kernel's; inside its repeats' spread ({u8[1] * 1e3:.1f} .. {u8[2] * 1e3:.1f}): {u8[1] <= m <= u8[2]}"
            print(f"      {l0[f]:28s} {m * 1e3:7.1f} us = {m * 1e3 / per:5.2f} us/frame ({lo * 1e3:.1f} .. {hi * 1e3:.1f}){note}")
        # the camera loop, records + annotated raw frames back, 2 chunks per call
        m2 = 2 * B
        loop = lambda f, order: ctx.loop_images(imgs[f][:m2], pixfmt=f, precision="fp16", thresh=0.25, nms=0.45, batch=B, cap=100, out_order=order)
        cases = (("rgb24", "rgb"), ("rgb24", "bgr"), ("bgr24", "rgb"), ("bgr24", "bgr"), ("bgra32", "bgr"))
        want = loop("rgb24", "rgb")
        lt = {k: [] for k in cases}
        for k in cases:
            got = loop(*k)
            assert all(np.array_equal(a, b if k[1] == "rgb" else b[..., ::-1]) for a, b in zip(got["frames"][:16], want["frames"][:16])), k
        del got
        for _ in range(REPS):
            for k in cases:
                lt[k].append(clock(lambda: loop(*k)))
        print(f"    the loop (yolo2_hip_loop_images_pix, fp16, {m2} frames per call in chunks of {B}, records + raw annotated frames back):")
        for k in cases:
            print(f"      {k[0].upper():6s} in, {k[1].upper()}24 out ({'k_annotate_batch_bgr' if k[1] == 'bgr' else 'k_annotate_batch'}): {fmt_rate(m2, lt[k])}")
        del want
    del imgs
ctx.close()
ctx8.close()
