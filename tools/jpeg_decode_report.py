#!/usr/bin/env python3
"""JPEG streams to detection records with the decoder on the host pool (the route before the GPU decoder existed) beside the decoder on
the GPU, in one process (GPU box):
  (a) y2h_decode_image on 16 threads (the CPU share of a job on the GPU machines), then yolo2_hip_run_images_pix_dets_f16 (fp16) or
      yolo2_hip_run_images_pix_dets (int16) on the decoded RGB24 frames;
  (b) yolo2_hip_run_images_jpeg_dets on the same streams;
  (c) route (b) under option jpegdec_split = S (many lanes per restart interval: k_jpegdec_split + k_jpegdec_rest), S in 64, 128, 256, 512.
Streams: dog.jpg as it is (768x576, h1v2, DRI 96: 36 restart intervals, so 36 lanes of k_jpegdec_entropy per frame), and the same
picture written by y2h_write_jpg_rgb24 at quality 80 (4:4:4, no DRI: one lane per frame).  Batches 64 and 256.  Every figure: one
warm-up call of the shape, then `reps` windows that end in a device synchronise; the two routes alternate inside a repeat and every
repeat is printed.  Also: device-event time of the decoder's kernels per chunk, staged / uploaded bytes per frame of both routes, and
the decode-only rate of yolo2_hip_decode_jpeg_host against the host pool.  The bar (DRI stream, batch 256): the median of (b) is not
below the median of (a) by more than the spread of (a)'s own repeats; the same bar for the best (c) on the stream without DRI at batch
256, against the (a) and (b) of the same run.  Per S also the event time of the two launches per chunk and the rounds.  Writes
profiles/r17_jpeg_split_rates.txt (profiles/r15_jpeg_decode_rates.txt is this tool's output before route (c) existed).
usage: python3 tools/jpeg_decode_report.py [chunks per call = 4] [reps = 3] [out = profiles/r17_jpeg_split_rates.txt]"""
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

CHUNKS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r17_jpeg_split_rates.txt")
THREADS = 16
SPLITS = (64, 128, 256, 512)

H = hipdrv.host_lib()
H.y2h_decode_image.restype = C.c_long
H.y2h_decode_image.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
L = hipdrv.lib()
lines = [f"JPEG streams -> records: host decode pool ({THREADS} threads) + _pix_dets entry (a) beside yolo2_hip_run_images_jpeg_dets (b) and the same under option jpegdec_split = S (c), one process; "
         f"{CHUNKS} chunks per call, {REPS} repeats after one warm-up call per shape, windows end in a device synchronise", ""]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


images = np.load(os.path.join(ROOT, "tests", "golden", "images.npz"))
dog = images["ref/dog.jpg/file"].tobytes()
W, Hh = 768, 576
dog_rgb = np.zeros((Hh, W, 3), dtype=np.uint8)
ww, hh = C.c_int(0), C.c_int(0)
assert H.y2h_decode_image(dog, len(dog), C.byref(ww), C.byref(hh), dog_rgb.ctypes.data_as(C.c_void_p), dog_rgb.size) == dog_rgb.size
plain = hipdrv.write_jpg_host(dog_rgb, 80)
STREAMS = {"dog.jpg (h1v2, DRI 96: 36 segments per frame)": dog, "dog re-encoded q80 (4:4:4, no DRI: 1 segment per frame)": plain}
for name, s in STREAMS.items():
    info = hipdrv.jpeg_probe(s)
    assert info["gpu_decodable"] and (info["width"], info["height"]) == (W, Hh), (name, info)

model = synth.SynthModel(seed=1)
ctx = hipdrv.Yolo2Hip(0)
ctx.load_model(model)
ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
pool = ThreadPoolExecutor(THREADS)
vp = lambda a: a.ctypes.data_as(C.c_void_p)
CAP = 100
verdict = None
split_verdict = None

for B in (64, 256):
    n = CHUNKS * B
    frames = np.zeros((n, Hh, W, 3), dtype=np.uint8)              # route (a)'s decoded frames, every one written by every call
    fptrs = (C.c_void_p * n)(*[frames[i].ctypes.data for i in range(n)])
    ws, hs = (C.c_int * n)(*([W] * n)), (C.c_int * n)(*([Hh] * n))
    dets = np.zeros((n, CAP), dtype=hipdrv.DET_DTYPE)
    counts, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    jw, jh = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    q = C.c_int(0)
    for sname, stream in STREAMS.items():
        buf = C.create_string_buffer(stream, len(stream))
        sptrs = (C.c_void_p * n)(*([C.addressof(buf)] * n))
        sizes = (C.c_size_t * n)(*([len(stream)] * n))

        def host_decode():
            def part(t):
                w1, h1 = C.c_int(0), C.c_int(0)
                for i in range(t, n, THREADS):
                    assert H.y2h_decode_image(stream, len(stream), C.byref(w1), C.byref(h1), fptrs[i], W * Hh * 3) == W * Hh * 3
            list(pool.map(part, range(THREADS)))

        say(f"batch {B}, {sname}: {len(stream)} bytes per stream, {n} frames per call")
        for prec, code in (("fp16", 1), ("int16", 0)):
            def route_a():
                host_decode()
                if prec == "fp16":
                    rc = L.yolo2_hip_run_images_pix_dets_f16(ctx._h, 0, fptrs, ws, hs, 3, n, B, 0.25, 0.45, 1, vp(dets), CAP, vp(counts))
                else:
                    rc = L.yolo2_hip_run_images_pix_dets(ctx._h, fptrs, ws, hs, 3, n, B, 0.25, 0.45, 1, vp(dets), CAP, vp(counts), C.byref(q))
                hipdrv.check(rc, "route (a)")

            def route_b():
                hipdrv.check(L.yolo2_hip_run_images_jpeg_dets(ctx._h, code, sptrs, sizes, vp(jw), vp(jh), n, B, 0.25, 0.45, 1, vp(dets), CAP, vp(counts),
                                                              C.byref(q), vp(status)), "route (b)")

            def route_c(S):
                ctx.set_option("jpegdec_split", S)
                try:
                    route_b()
                finally:
                    ctx.set_option("jpegdec_split", None)

            route_a()
            want = counts.copy()
            route_b()
            assert np.array_equal(counts, want) and not status.any()           # the two routes return the same records
            for S in SPLITS:
                route_c(S)
                assert np.array_equal(counts, want) and not status.any()       # ... and so does every (c)
            t = {"a": [], "b": []}
            t.update({S: [] for S in SPLITS})
            for _ in range(REPS):
                t["a"].append(window(route_a))
                t["b"].append(window(route_b))
                for S in SPLITS:
                    t[S].append(window(lambda: route_c(S)))
            ra, rb = [n / x for x in t["a"]], [n / x for x in t["b"]]
            ma, mb = statistics.median(ra), statistics.median(rb)
            say(f"  {prec}: (a) host pool + pix entry: median {ma:.0f} frames/s (repeats {', '.join(f'{r:.0f}' for r in ra)}); "
                f"(b) GPU decoder: median {mb:.0f} frames/s (repeats {', '.join(f'{r:.0f}' for r in rb)}); (b) / (a) = {mb / ma:.2f}")
            rc_ = {S: [n / x for x in t[S]] for S in SPLITS}
            mc = {S: statistics.median(rc_[S]) for S in SPLITS}
            for S in SPLITS:
                say(f"    (c) S = {S}: median {mc[S]:.0f} frames/s (repeats {', '.join(f'{r:.0f}' for r in rc_[S])}); (c) / (b) = {mc[S] / mb:.2f}, "
                    f"(c) / (a) = {mc[S] / ma:.2f}")
            if B == 256 and "no DRI" in sname:
                best = max(SPLITS, key=lambda S: mc[S])
                spread = max(ra) - min(ra)
                ok = mc[best] >= ma - spread
                split_verdict = (split_verdict or []) + [f"{prec}: best (c) S = {best}: {mc[best]:.0f} against (a) {ma:.0f} - spread {spread:.0f} frames/s, "
                                                         f"(b) {mb:.0f}: {'met' if ok else 'NOT met'}"]
            if B == 256 and "DRI 96" in sname:
                spread = max(ra) - min(ra)
                ok = mb >= ma - spread
                verdict = (verdict or []) + [f"{prec}: (b) {mb:.0f} against (a) {ma:.0f} - spread {spread:.0f} frames/s: {'met' if ok else 'NOT met'}"]
        # per-kernel device time and uploaded bytes of route (b), one call under profiling (fp16)
        ctx.set_profiling(True)
        hipdrv.check(L.yolo2_hip_run_images_jpeg_dets(ctx._h, 1, sptrs, sizes, vp(jw), vp(jh), n, B, 0.25, 0.45, 1, vp(dets), CAP, vp(counts), C.byref(q),
                                                      vp(status)), "profiled call")
        ctx.set_profiling(False)
        i = hipdrv.jpeg_last_info(ctx._h)
        dec_ms = i["memset_ms"] + i["entropy_ms"] + i["idct_ms"] + i["rgb_ms"]
        say(f"  decoder kernels per chunk of {B} (device events, mean of {i['chunks']} chunks): coefficient memset {i['memset_ms']:.3f} ms, "
            f"k_jpegdec_entropy {i['entropy_ms']:.3f} ms, k_jpegdec_idct {i['idct_ms']:.3f} ms, k_jpegdec_rgb (+ _zero) {i['rgb_ms']:.3f} ms; "
            f"sum {dec_ms:.3f} ms = {B / (dec_ms * 1e-3):.0f} frames/s if nothing else ran")
        say(f"  bytes per frame: (a) staged and uploaded {W * Hh * 3} (raw RGB24); (b) staged and uploaded {i['stream_bytes_h2d'] / n:.0f} "
            f"(streams, descriptors, tables) + {i['frame_bytes_h2d'] / n:.0f} (letterbox table) = {(i['stream_bytes_h2d'] + i['frame_bytes_h2d']) / n / (W * Hh * 3):.3f} of (a)")
        for S in SPLITS:
            ctx.set_option("jpegdec_split", S)
            ctx.set_profiling(True)
            hipdrv.check(L.yolo2_hip_run_images_jpeg_dets(ctx._h, 1, sptrs, sizes, vp(jw), vp(jh), n, B, 0.25, 0.45, 1, vp(dets), CAP, vp(counts), C.byref(q),
                                                          vp(status)), "profiled split call")
            ctx.set_profiling(False)
            ctx.set_option("jpegdec_split", None)
            i, k = hipdrv.jpeg_last_info(ctx._h), hipdrv.jpeg_split_info(ctx._h)
            say(f"  jpegdec_split = {S}, per chunk of {B}: k_jpegdec_split {k['split_ms']:.3f} ms + k_jpegdec_rest {k['fallback_ms']:.3f} ms (entropy stage "
                f"{i['entropy_ms']:.3f} ms); per call {k['subsequences']} subsequences, {k['split_segments']} segments split, {k['fallback_segments']} fell back, "
                f"{k['short_segments']} too short, most rounds of a segment {k['max_rounds']}")
        # decode only
        outs = (C.c_void_p * n)(*[frames[k].ctypes.data for k in range(n)])
        caps = (C.c_size_t * n)(*([W * Hh * 3] * n))
        gpu_decode = lambda: hipdrv.check(L.yolo2_hip_decode_jpeg_host(ctx._h, sptrs, sizes, n, B, outs, caps, vp(jw), vp(jh), vp(status)), "decode entry")
        gpu_decode()
        assert np.array_equal(frames[0], dog_rgb) if stream is dog else True
        td, th = [], []
        for _ in range(REPS):
            th.append(window(host_decode))
            td.append(window(gpu_decode))
        say(f"  decode only (streams in host memory -> RGB24 in host memory): host pool median {n / statistics.median(th):.0f} frames/s; "
            f"yolo2_hip_decode_jpeg_host median {n / statistics.median(td):.0f} frames/s (its D2H and copy-out move {W * Hh * 3} bytes per frame)")
    del frames
    say()

say("bar (DRI stream at batch 256: median of (b) not below the median of (a) by more than the spread of (a)'s repeats):")
for v in verdict or ["not measured"]:
    say("  " + v)
say("the same bar for route (c) on the stream without DRI at batch 256 (best S; (a) and (b) of the same repeats):")
for v in split_verdict or ["not measured"]:
    say("  " + v)
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(text)
ctx.close()
