#!/usr/bin/env python3
"""The camera loop from JPEG streams, in one process (GPU box): records and annotated frames from
  (a) the route callers had before: y2h_decode_image on 16 threads (the CPU share of a job on the GPU machines), then
      yolo2_hip_loop_images_pix on the decoded RGB24 frames;
  (b) yolo2_hip_loop_images_jpeg on the same streams, option jpegdec_split unset;
  (c) route (b) under jpegdec_split = S, S in 64, 128.
Streams: dog.jpg as it is (768x576, h1v2, DRI 96) and the same picture written by y2h_write_jpg_rgb24 at quality 80 (4:4:4, no DRI).
Configurations: int16 at batch 64 and fp16 at batch 256, each with JPEG out at quality 80 and with RGB24 out.  Every figure: one warm-up
call of the shape, then `reps` windows that end in a device synchronise; the routes alternate inside a repeat; median with min - max.
Also: bytes uploaded and downloaded per frame by both routes (yolo2_hip_loop_last_info), the decoder's per-chunk device-event times
(yolo2_hip_jpeg_last_info / _split_info under yolo2_hip_set_profiling), and the latency of a call at n = 1 (median of 50 calls, both
routes): a live camera runs the loop frame by frame.  No bar is set here; every ratio is printed, including those below 1.
Writes profiles/r18_jpeg_loop_rates.txt.
usage: python3 tools/jpeg_loop_report.py [chunks per call = 2] [reps = 3] [out = profiles/r18_jpeg_loop_rates.txt]"""
import ctypes as C
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
import numpy as np
import torch
from yolo2_amd import hipdrv, synth

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 2
REPS = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r18_jpeg_loop_rates.txt")
THREADS = 16
SPLITS = (64, 128)
CAP, THRESH, NMS, QUALITY = 845, 0.24, 0.45, 80
FLAGS = hipdrv.DETS_BEST_CLASS | hipdrv.DETS_APP_TAIL

H = hipdrv.host_lib()
H.y2h_decode_image.restype = C.c_long
H.y2h_decode_image.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
L = hipdrv.lib()
lines = [f"camera loop from JPEG streams: host decode pool ({THREADS} threads) + yolo2_hip_loop_images_pix (a) beside yolo2_hip_loop_images_jpeg (b) and the "
         f"same under option jpegdec_split = S (c), one process; {CHUNKS} chunks per call, {REPS} repeats after one warm-up call per shape, windows end in "
         f"a device synchronise; thresh {THRESH}, app tail, labels of coco.names", ""]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def mmm(v):
    return f"median {statistics.median(v):.0f} (min {min(v):.0f} - max {max(v):.0f})"


images = np.load(os.path.join(ROOT, "tests", "golden", "images.npz"))
dog = images["ref/dog.jpg/file"].tobytes()
W, Hh = 768, 576
RAW = W * Hh * 3
dog_rgb = np.zeros((Hh, W, 3), dtype=np.uint8)
ww, hh = C.c_int(0), C.c_int(0)
assert H.y2h_decode_image(dog, len(dog), C.byref(ww), C.byref(hh), dog_rgb.ctypes.data_as(C.c_void_p), dog_rgb.size) == dog_rgb.size
plain = hipdrv.write_jpg_host(dog_rgb, 80)
STREAMS = {"dog.jpg (h1v2, DRI 96: 36 segments per frame)": dog, "dog re-encoded q80 (4:4:4, no DRI: 1 segment per frame)": plain}
names = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
lab, n_labels, _keep_labels = hipdrv._label_args(names)

model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
pool = ThreadPoolExecutor(THREADS)
vp = lambda a: a.ctypes.data_as(C.c_void_p)
OUT_CAP = max(RAW, hipdrv.jpeg_bound(W, Hh))


class Shape:
    """the buffers of calls on n frames at batch B"""

    def __init__(self, n, B):
        self.n, self.B = n, B
        self.frames = np.zeros((n, Hh, W, 3), dtype=np.uint8)          # route (a)'s decoded frames, every one written by every call
        self.fptrs = (C.c_void_p * n)(*[self.frames[i].ctypes.data for i in range(n)])
        self.ws, self.hs = (C.c_int * n)(*([W] * n)), (C.c_int * n)(*([Hh] * n))
        self.jw, self.jh = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        self.dets = np.zeros((n, CAP), dtype=hipdrv.DET_DTYPE)
        self.counts, self.status, self.drawn = (np.zeros(n, dtype=np.int32) for _ in range(3))
        self.outs = np.zeros((n, OUT_CAP), dtype=np.uint8)
        self.optrs = (C.c_void_p * n)(*[self.outs[i].ctypes.data for i in range(n)])
        self.caps = np.full(n, OUT_CAP, dtype=np.uint64)
        self.sizes = np.zeros(n, dtype=np.uint64)
        self.q = C.c_int(0)

    def stream(self, data):
        self.data = data
        self.buf = C.create_string_buffer(data, len(data))
        self.sptrs = (C.c_void_p * self.n)(*([C.addressof(self.buf)] * self.n))
        self.ssizes = (C.c_size_t * self.n)(*([len(data)] * self.n))

    def host_decode(self):
        def part(t):
            w1, h1 = C.c_int(0), C.c_int(0)
            for i in range(t, self.n, THREADS):
                assert H.y2h_decode_image(self.data, len(self.data), C.byref(w1), C.byref(h1), self.fptrs[i], RAW) == RAW
        list(pool.map(part, range(min(THREADS, self.n))))

    def route_a(self, code, jpeg):
        self.host_decode()
        hipdrv.check(L.yolo2_hip_loop_images_pix(ctx._h, code, self.fptrs, self.ws, self.hs, 3, self.n, self.B, THRESH, NMS, FLAGS, vp(self.dets), CAP,
                                                 vp(self.counts), C.byref(self.q), lab, n_labels, int(jpeg), QUALITY, self.optrs, vp(self.caps),
                                                 vp(self.sizes), vp(self.drawn)), "route (a)")

    def route_b(self, code, jpeg, S=None):
        if S:
            ctx.set_option("jpegdec_split", S)
        try:
            hipdrv.check(L.yolo2_hip_loop_images_jpeg(ctx._h, code, self.sptrs, self.ssizes, vp(self.jw), vp(self.jh), self.n, self.B, THRESH, NMS, FLAGS,
                                                      vp(self.dets), CAP, vp(self.counts), C.byref(self.q), lab, n_labels, int(jpeg), QUALITY, self.optrs,
                                                      vp(self.caps), vp(self.sizes), vp(self.drawn), vp(self.status)), "route (b)")
        finally:
            if S:
                ctx.set_option("jpegdec_split", None)

    def result(self):
        return (self.counts.copy(), self.drawn.copy(), self.sizes.copy(), self.outs[0, :int(self.sizes[0])].tobytes(),
                self.outs[-1, :int(self.sizes[-1])].tobytes())


def same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


for prec, code, B in (("int16", 0, 64), ("fp16", 1, 256)):
    n = CHUNKS * B
    sh = Shape(n, B)
    for sname, data in STREAMS.items():
        sh.stream(data)
        say(f"{prec}, batch {B}, {sname}: {len(data)} bytes per stream, {n} frames per call")
        for jpeg in (True, False):
            out = f"JPEG out q{QUALITY}" if jpeg else "RGB24 out"
            sh.route_a(code, jpeg)
            want, pix = sh.result(), ctx.loop_last_info()
            sh.route_b(code, jpeg)
            assert same(sh.result(), want) and not sh.status.any()       # the routes return the same records and frames
            info, j = ctx.loop_last_info(), hipdrv.jpeg_last_info(ctx._h)
            for S in SPLITS:
                sh.route_b(code, jpeg, S)
                assert same(sh.result(), want) and not sh.status.any()
            t = {"a": [], "b": []}
            t.update({S: [] for S in SPLITS})
            for _ in range(REPS):
                t["a"].append(window(lambda: sh.route_a(code, jpeg)))
                t["b"].append(window(lambda: sh.route_b(code, jpeg)))
                for S in SPLITS:
                    t[S].append(window(lambda: sh.route_b(code, jpeg, S)))
            r = {k: [n / x for x in v] for k, v in t.items()}
            ma, mb = statistics.median(r["a"]), statistics.median(r["b"])
            say(f"  {out}: (a) host pool + pix loop: {mmm(r['a'])} frames/s; (b) loop from streams: {mmm(r['b'])} frames/s; (b) / (a) = {mb / ma:.2f}")
            for S in SPLITS:
                mc = statistics.median(r[S])
                say(f"    (c) S = {S}: {mmm(r[S])} frames/s; (c) / (b) = {mc / mb:.2f}, (c) / (a) = {mc / ma:.2f}")
            say(f"    bytes per frame: (a) staged {pix['image_bytes_staged'] / n:.0f}, uploaded {pix['image_bytes_h2d'] / n:.0f}, downloaded "
                f"{pix['out_bytes_d2h'] / n:.0f}; (b) staged {info['image_bytes_staged'] / n:.0f}, uploaded {info['image_bytes_h2d'] / n:.0f} "
                f"({j['stream_bytes_h2d'] / n:.0f} descriptors, tables and streams + {j['frame_bytes_h2d'] / n:.0f} letterbox, painter and encoder tables), "
                f"downloaded {info['out_bytes_d2h'] / n:.0f}; uploaded (b) / (a) = {info['image_bytes_h2d'] / pix['image_bytes_h2d']:.3f}")
        # the decoder's kernels per chunk, one call under profiling (JPEG out)
        ctx.set_profiling(True)
        sh.route_b(code, True)
        ctx.set_profiling(False)
        i = hipdrv.jpeg_last_info(ctx._h)
        dec_ms = i["memset_ms"] + i["entropy_ms"] + i["idct_ms"] + i["rgb_ms"]
        say(f"  decoder stages per chunk of {B} (device events, mean of {i['chunks']} chunks): coefficient memset {i['memset_ms']:.3f} ms, k_jpegdec_entropy "
            f"{i['entropy_ms']:.3f} ms, k_jpegdec_idct {i['idct_ms']:.3f} ms, k_jpegdec_rgb (+ _zero) {i['rgb_ms']:.3f} ms; sum {dec_ms:.3f} ms")
        for S in SPLITS:
            ctx.set_profiling(True)
            sh.route_b(code, True, S)
            ctx.set_profiling(False)
            i, k = hipdrv.jpeg_last_info(ctx._h), hipdrv.jpeg_split_info(ctx._h)
            say(f"  jpegdec_split = {S}, per chunk of {B}: k_jpegdec_split {k['split_ms']:.3f} ms + k_jpegdec_rest {k['fallback_ms']:.3f} ms (entropy stage "
                f"{i['entropy_ms']:.3f} ms); per call {k['split_segments']} segments split, {k['fallback_segments']} fell back, {k['short_segments']} too short")
        say()
    del sh

say("latency of one call at n = 1 (median of 50 calls after a warm-up call, milliseconds; (a) = one y2h_decode_image + the pix loop):")
for prec, code in (("int16", 0), ("fp16", 1)):
    sh = Shape(1, 1)
    for sname, data in STREAMS.items():
        sh.stream(data)
        for jpeg in (True, False):
            sh.route_a(code, jpeg)
            want = sh.result()
            sh.route_b(code, jpeg)
            assert same(sh.result(), want) and not sh.status.any()
            routes = [("a", lambda: sh.route_a(code, jpeg)), ("b", lambda: sh.route_b(code, jpeg))] + [(S, (lambda S: lambda: sh.route_b(code, jpeg, S))(S))
                                                                                                      for S in SPLITS]
            for _, fn in routes[2:]:
                fn()
            t = {k: [] for k, _ in routes}
            for _ in range(50):
                for k, fn in routes:
                    t[k].append(window(fn) * 1e3)
            med = {k: statistics.median(v) for k, v in t.items()}
            say(f"  {prec}, {sname.split(' (')[0]}, {'JPEG out' if jpeg else 'RGB24 out'}: (a) {med['a']:.2f} (min {min(t['a']):.2f} - max {max(t['a']):.2f}); "
                f"(b) {med['b']:.2f} (min {min(t['b']):.2f} - max {max(t['b']):.2f}); (a) / (b) = {med['a'] / med['b']:.2f}; " +
                "; ".join(f"S = {S}: {med[S]:.2f}, (a) / (c) = {med['a'] / med[S]:.2f}" for S in SPLITS))
    del sh
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
ctx.close()
