"""Harness of the caller-stream tests (tests/test_gpu_streams.py, tests/test_streams_host.py).

include/yolo2_hip.h promises of every entry that takes a `void *stream` that its work is ordered on that stream: an `enqueue` entry
returns without synchronising, a `sync` entry synchronises the stream before it returns, and internal lanes are forked from and
joined to it.  On the null stream none of that can be seen to fail, since the null stream orders against everything.  Here the
entry runs on a non-blocking stream whose input arrives LATE (behind a delay of measured length, until which the buffer holds another
valid input, the poison) and is overwritten EARLY (right behind the call, on the same stream): work that escaped the stream, or a lane
that was not joined, reads the poison or is copied out half-written, and the bit-exact passes turn that into different bits.

torch.cuda supplies device memory, streams and events, as in bench.py; the entries are called through yolo2_amd.hipdrv."""
import ctypes as C
import math
import os
import time

import numpy as np
# torch comes with a HIP runtime of its own.  Imported here, i.e. when pytest collects, before anything has loaded libyolo2_hip.so,
# the library binds to that same runtime, as it does in bench.py; the other way round the process holds two runtimes and torch.cuda
# finds no device.
import torch

# one row per `void *stream` prototype of include/yolo2_hip.h (tests/test_streams_host.py holds the two together)
ENTRIES = {
    "yolo2_hip_run_batch_int16": "enqueue",
    "yolo2_hip_run_batch_fp16": "enqueue",
    "yolo2_hip_run_batch_f32tol": "enqueue",
    "yolo2_hip_run_batch_fp32": "enqueue",
    "yolo2_hip_run_batch_int8": "enqueue",
    "yolo2_hip_letterbox_u8": "enqueue",
    "yolo2_hip_letterbox_pix": "enqueue",
    "yolo2_hip_postprocess_int16": "sync",
    "yolo2_hip_postprocess_f32": "sync",
    "yolo2_hip_postprocess_int16_app": "sync",
    "yolo2_hip_postprocess_f32_app": "sync",
    "yolo2_hip_annotate_pix": "sync",
    "yolo2_hip_jpeg_encode_rgb24": "sync",
    "yolo2_hip_absmax_f32": "sync",
    "yolo2_hip_calib_frames": "sync",
}

FILL = 0x5A                      # what an output buffer holds before a call: a store that never happened shows
DELAY_FACTOR = 20                # the delay is at least this many times the host's time to enqueue the call ...
DELAY_FLOOR_MS = 1.0             # ... at least the call's own device time, and at least this
DELAY_MARGIN = 1.25             # copies are enqueued for this much more: the copy time was measured once and clocks move
DELAY_MAX_COPIES = 8000


def side_stream(avoid=()):
    """A stream of the caller's own.  torch creates its streams non-blocking, i.e. without implicit ordering against the null
    stream.  HIP, however, multiplexes its streams onto a few hardware queues, and two streams that share one run
    in order whatever their flags: a launch that escaped to the null stream would then still sit behind the delay and go unnoticed.
    So a candidate is taken only once work on the null stream - and on every stream of `avoid` - has been seen to finish while a
    delay on the candidate was still running.  The negative control of tests/test_gpu_streams.py proves the whole arrangement."""
    others = [torch.cuda.default_stream()] + list(avoid)
    for _ in range(32):
        s = torch.cuda.Stream()
        if all(s.cuda_stream != o.cuda_stream and runs_beside(s, o) for o in others):
            return s
    raise AssertionError("no stream torch hands out runs beside the null stream and " + str(list(avoid)) + ": nothing can be shown here")


def runs_beside(s, other, ms=2.0):
    """work enqueued on `other` finishes while a delay of `ms` on `s` is still running"""
    torch.cuda.synchronize()
    d = delay()
    _, end = d.enqueue(s, ms)
    done = torch.cuda.Event()
    with torch.cuda.stream(other):
        d.probe[1].copy_(d.probe[0], non_blocking=True)
        done.record(other)
    done.synchronize()
    beside = not end.query()
    s.synchronize()
    return beside


class Delay:
    """Device work of known length on a stream: a chain of device-to-device copies between two large tensors, the time of one copy
    measured once per process with an event pair."""

    CHUNK = 1 << 30

    def __init__(self):
        self.a = torch.zeros(self.CHUNK, dtype=torch.uint8, device="cuda")
        self.b = torch.zeros(self.CHUNK, dtype=torch.uint8, device="cuda")
        self.probe = torch.zeros(2, 256, dtype=torch.uint8, device="cuda")       # (runs_beside's few bytes of work)
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            for _ in range(4):
                self.b.copy_(self.a, non_blocking=True)
            e0.record(s)
            for _ in range(16):
                self.b.copy_(self.a, non_blocking=True)
            e1.record(s)
        s.synchronize()
        self.ms_per_copy = e0.elapsed_time(e1) / 16
        assert self.ms_per_copy > 0.05, f"a {self.CHUNK >> 20} MiB copy in {self.ms_per_copy} ms: the event pair did not measure it"

    @staticmethod
    def length_ms(t_enqueue_s, t_device_s):
        """the delay an entry needs: DELAY_FACTOR x its host time, and no less than its device time"""
        return max(DELAY_FACTOR * t_enqueue_s * 1e3, t_device_s * 1e3, DELAY_FLOOR_MS)

    def enqueue(self, stream, ms):
        """-> (event before the chain, event behind it), both timed"""
        n = int(math.ceil(DELAY_MARGIN * ms / self.ms_per_copy)) + 1
        assert n <= DELAY_MAX_COPIES, f"a delay of {ms:.1f} ms takes {n} copies: the entry's host time was mismeasured"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(n):
                self.b.copy_(self.a, non_blocking=True)
            e1.record(stream)
        return e0, e1


_delay = None


def delay():
    global _delay
    if _delay is None:
        _delay = Delay()
    return _delay


def late_input(stream, buf, true_dev, poison_dev, ms=DELAY_FLOOR_MS):
    """`buf` holds the poison now; on `stream`: a delay of `ms`, then the true input.  -> (event before the delay, event behind it)"""
    buf.copy_(poison_dev)
    torch.cuda.synchronize()
    e0, e1 = delay().enqueue(stream, ms)
    with torch.cuda.stream(stream):
        buf.copy_(true_dev, non_blocking=True)
    return e0, e1


def drain_and_clobber(stream, out_buf, pinned_host, in_buf, poison_dev):
    """On `stream`: the output to pinned host memory, then the poison over the input again."""
    with torch.cuda.stream(stream):
        if out_buf is not None:
            pinned_host.copy_(out_buf, non_blocking=True)
        in_buf.copy_(poison_dev, non_blocking=True)


def dev(arr):
    """a numpy array's bytes as a uint8 tensor in device memory (a blocking upload)"""
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def out_bufs(nbytes):
    """(device output filled with FILL, pinned host tensor of the same size) - or (None, None) for an entry without a device output"""
    if not nbytes:
        return None, None
    out = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    pin = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
    return out, pin


def ptr(t):
    return t.data_ptr() if t is not None else 0


def same(a, b):
    """bitwise equality of two lists of arrays"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def log(entry, label, scenario, t_enqueue_s, delay_ms, verdict, note=""):
    """one line per case - and the harness's own promise: the delay that ran (event time) was DELAY_FACTOR x t_enqueue or more"""
    line = (f"{entry} {label} scenario={scenario} t_enqueue_ms={t_enqueue_s * 1e3:.4f} delay_ms={delay_ms:.3f} "
            f"ratio={delay_ms / max(t_enqueue_s * 1e3, 1e-9):.1f} {verdict}{' ' + note if note else ''}")
    print(line)
    p = os.environ.get("YOLO2_STREAM_LOG")
    if p:
        with open(p, "a") as f:
            f.write(line + "\n")
    assert delay_ms >= DELAY_FACTOR * t_enqueue_s * 1e3, \
        f"inconclusive: the delay ran {delay_ms:.3f} ms, under {DELAY_FACTOR} x the {t_enqueue_s * 1e3:.4f} ms the host needs to enqueue {entry}"


# ------------------------------------------------------------------ the cases: an entry at one shape

class Case:
    """entry: symbol name; label: the shape; true / poison: two valid inputs of one size (numpy); out_nbytes: size of the device
    output (0: none); call(ctx, in_ptr, out_ptr, stream) -> list of host-side results (numpy); view(out_bytes, host) -> the arrays
    that are compared; check(ctx): asserted on the context after a run (lane counts); anchor(values): asserted on the null-stream
    values (frame 0 against a fixture)."""

    def __init__(self, entry, label, true, poison, out_nbytes, call, view=None, check=None, anchor=None):
        assert true.shape == poison.shape and true.dtype == poison.dtype and true.tobytes() != poison.tobytes()
        self.entry, self.label, self.kind = entry, label, ENTRIES[entry]
        self.true, self.poison, self.out_nbytes, self.call = true, poison, out_nbytes, call
        self.view = view or (lambda out, host: ([out] if out is not None else []) + list(host))
        self.check, self.anchor = check, anchor

    @property
    def key(self):
        return (self.entry, self.label)


class Expected:
    def __init__(self, values, t_enqueue, t_device):
        self.values, self.t_enqueue, self.t_device = values, t_enqueue, t_device


_expected = {}


def expected(case, ctx):
    """The case through the same entry on the NULL stream of `ctx` (a context no side-stream call ever uses), followed by a device
    synchronise: the values, the host wall time of the warmed call (t_enqueue) and of the call plus its device work (t_device)."""
    if case.key in _expected:
        return _expected[case.key]
    buf = dev(case.true)
    out, _ = out_bufs(case.out_nbytes)
    case.call(ctx, ptr(buf), ptr(out), 0)            # warms: plans, tables, the batch's tensors
    torch.cuda.synchronize()
    if out is not None:
        out.fill_(FILL)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = case.call(ctx, ptr(buf), ptr(out), 0)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    values = case.view(out.cpu().numpy() if out is not None else None, host)
    if case.check:
        case.check(ctx)
    if case.anchor:
        case.anchor(values)
    e = _expected[case.key] = Expected(values, t1 - t0, t2 - t0)
    return e


def scenario_a(case, ctx, ref_ctx, call_stream=None, scenario="A"):
    """Late input, early clobber: late_input on a side stream, the call (on that stream, or - the negative control - on
    `call_stream`), drain_and_clobber, one synchronise.  -> (got == expected bitwise, the delay's end event was complete when the
    call returned)"""
    exp = expected(case, ref_ctx)
    s = side_stream(avoid=[call_stream] if call_stream is not None and call_stream.cuda_stream else ())
    cs = s if call_stream is None else call_stream
    cs_int = cs.cuda_stream
    true_d, poison_d = dev(case.true), dev(case.poison)
    buf = poison_d.clone()
    out, pin = out_bufs(case.out_nbytes)
    if case.kind == "enqueue":                       # planning syncs of a first call at this batch are out of the way
        case.call(ctx, ptr(buf), ptr(out), cs_int)
        torch.cuda.synchronize()
        if out is not None:
            out.fill_(FILL)
    ms = Delay.length_ms(exp.t_enqueue, exp.t_device)
    e0, e1 = late_input(s, buf, true_d, poison_d, ms)
    host = case.call(ctx, ptr(buf), ptr(out), cs_int)
    done = e1.query()
    drain_and_clobber(s, out, pin, buf, poison_d)
    s.synchronize()
    if cs is not s:
        torch.cuda.synchronize()
    if case.check:
        case.check(ctx)
    got = case.view(pin.numpy().copy() if pin is not None else None, host)
    equal = same(got, exp.values)
    log(case.entry, case.label, scenario, exp.t_enqueue, e0.elapsed_time(e1), "equal" if equal else "differ",
        f"delay_done_on_return={int(done)}")
    return equal, done


# ------------------------------------------------------------------ inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pool = None


def frame_pool():
    """five distinct frames; frame 0 is the frame of tests/golden/fullnet.npz"""
    global _pool
    if _pool is None:
        from yolo2_amd import synth
        full = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))
        _pool = synth.frames(int(full["meta/frame_seed"]), 5)
    return _pool


def frames_for(batch, k=0):
    """input number k at a batch: frame i is pool frame (i + k) mod 5, so inputs k and k + 1 differ in every frame"""
    return np.ascontiguousarray(frame_pool()[(np.arange(batch) + k) % 5])


NET_ENTRIES = {"int16": "yolo2_hip_run_batch_int16", "fp16": "yolo2_hip_run_batch_fp16", "f32tol": "yolo2_hip_run_batch_f32tol",
               "fp32": "yolo2_hip_run_batch_fp32", "int8": "yolo2_hip_run_batch_int8"}


def net_case(prec, batch, k=0, lanes=None):
    """a network pass at a batch on input number k (the poison is input k + 1); lanes: the lane count the context must report"""
    full = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))

    def call(ctx, i, o, st):
        if prec == "int16":
            return [np.array([ctx.run_batch_ptr(i, batch, o, st)], dtype=np.int32)]
        {"fp16": ctx.run_batch_fp16_ptr, "f32tol": ctx.run_batch_f32tol_ptr, "fp32": ctx.run_batch_fp32_ptr,
         "int8": ctx.run_batch_int8_ptr}[prec](i, batch, o, st)
        return []

    def check(ctx):
        if lanes is not None:
            n = {"int16": ctx.num_lanes, "fp16": ctx.num_lanes_fp16, "f32tol": ctx.num_lanes_f32tol}[prec]()
            assert n == lanes, f"{prec} at batch {batch} runs {n} lane(s), the case is about {lanes}"

    def anchor(values):
        if k != 0 or prec not in ("int16", "fp32"):
            return
        n = 425 * 169
        if prec == "int16":
            assert int(values[1][0]) == int(full["i16/std/final_q"])
            assert np.array_equal(values[0][:n * 2].view(np.int16), full["i16/std/region_raw_i16"]), "frame 0 differs from the fixture"
        else:
            assert np.array_equal(values[0][:n * 4].view(np.uint32), full["f32/std/region_raw_f32"].view(np.uint32)), \
                "frame 0 differs from the fixture"

    item = 2 if prec == "int16" else 4
    return Case(NET_ENTRIES[prec], f"batch={batch}" + (f" input={k}" if k else ""), frames_for(batch, k), frames_for(batch, k + 1),
                batch * 425 * 169 * item, call, check=check, anchor=anchor)


def _lib():
    from yolo2_amd import hipdrv
    return hipdrv, hipdrv.lib()


def letterbox_case(entry, name, image, poison, fmt, net=416, want=None):
    """fmt: channels (1 / 3) for yolo2_hip_letterbox_u8, a YOLO2_PIX_* code for yolo2_hip_letterbox_pix; want: the fixture's frame"""
    h, w = image.shape[:2]

    def call(ctx, i, o, st):
        hipdrv, L = _lib()
        hipdrv.check(getattr(L, entry)(i, w, h, fmt, o, net, net, C.c_void_p(st)), entry)
        return []

    def anchor(values):
        if want is not None:
            assert np.array_equal(values[0].view(np.uint32), want.reshape(-1).view(np.uint32)), "the frame differs from the fixture"

    return Case(entry, name, image, poison, 3 * net * net * 4, call, anchor=anchor)


def letterbox_cases():
    hipdrv, _ = _lib()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "host.npz"))
    rng = np.random.default_rng(57)
    rgb = np.ascontiguousarray(np.moveaxis(fx["letterbox/57x41to96x96/in"], 0, 2))               # 57 wide, 41 high
    grey = np.ascontiguousarray(fx["letterbox/33x80to96x96/in"][1])                              # 33 wide, 80 high
    other = lambda a: rng.integers(0, 256, a.shape, dtype=np.uint8)
    y2, y640 = other(np.empty((2, 2, 2))), other(np.empty((480, 640, 2)))
    P = hipdrv.PIXFMTS
    want = fx["letterbox/57x41to96x96/out"]
    return [letterbox_case("yolo2_hip_letterbox_u8", "57x41 rgb", rgb, other(rgb), 3, 96, want),
            letterbox_case("yolo2_hip_letterbox_u8", "33x80 grey", grey, other(grey), 1),
            letterbox_case("yolo2_hip_letterbox_pix", "57x41 rgb24", rgb, other(rgb), P["rgb24"], 96, want),
            letterbox_case("yolo2_hip_letterbox_pix", "33x80 grey8", grey, other(grey), P["grey8"]),
            letterbox_case("yolo2_hip_letterbox_pix", "2x2 yuyv", y2, other(y2), P["yuyv"]),
            letterbox_case("yolo2_hip_letterbox_pix", "640x480 yuyv", y640, other(y640), P["yuyv"])]


TAIL_Q = 9


def tail_cases():
    """the four tails at batch 3: frame 0 is the tensor of tests/golden/host.npz detect/*, frames 1 and 2 are rotations of it; the
    poison is three other rotations; rows, totals, proc and the records are all asked for"""
    import orclib
    hipdrv, _ = _lib()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "host.npz"))
    raw = fx["detect/raw"]
    ri = np.rint(raw * (1 << TAIL_Q)).astype(np.int16)
    assert np.array_equal(ri.astype(np.float32) * np.float32(2.0 ** -TAIL_Q), raw)
    imw, imh, thresh, nms = fx["detect/std/params"]
    ws, hs = [int(imw), 500, 333], [int(imh), 375, 999]
    true = np.stack([ri, np.roll(ri, 169 * 7), np.roll(ri, 169 * 90 + 5)])
    poison = np.stack([np.roll(ri, 169 * 40), np.roll(ri, 3), np.roll(ri, 169 * 200)])
    cases = []
    for name, is_int, tail in (("postprocess_int16", True, "core"), ("postprocess_f32", False, "core"),
                               ("postprocess_int16_app", True, "app"), ("postprocess_f32_app", False, "app")):
        def call(ctx, i, o, st, is_int=is_int, tail=tail):
            r = hipdrv.postprocess(ctx, i, 3, ws, hs, float(thresh), float(nms), final_q=TAIL_Q if is_int else None, cap=2048,
                                   want_rows=True, want_proc=True, stream=st, tail=tail)
            recs = np.concatenate(r["dets"]) if sum(len(d) for d in r["dets"]) else np.zeros(0, dtype=hipdrv.DET_DTYPE)
            return [r["counts"], r["totals"], r["rows"], r["proc"], recs.view(np.uint8)]

        def anchor(values, is_int=is_int, tail=tail):
            counts, totals, rows, proc = values[:4]
            assert counts[0] > 0 and totals[0] > 0, "frame 0 gives no detection: the case compares nothing"
            if tail != "core":
                return            # (another arithmetic than the fixture's: tests/test_gpu_app_tail.py pins it to apptail.npz)
            got = orclib.canon_rows(rows[0])
            want = fx["detect/std/rows"]
            assert got.shape == want.shape
            if is_int:
                assert np.array_equal(proc[0].view(np.uint32), fx["detect/proc"].view(np.uint32))
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            else:                 # the float entry evaluates exp on the device: the bounds of tests/test_gpu_post_multi.py
                assert np.allclose(proc[0], fx["detect/proc"], rtol=2e-6, atol=1e-9) and np.allclose(got, want, rtol=1e-5, atol=1e-7)

        conv = (lambda a: a) if is_int else (lambda a: a.astype(np.float32) * np.float32(2.0 ** -TAIL_Q))
        cases.append(Case("yolo2_hip_" + name, "batch=3", conv(true), conv(poison), 0, call, anchor=anchor))
    return cases


def annotate_cases():
    import drawref
    import yuyvref
    hipdrv, _ = _lib()
    rng = np.random.default_rng(34)
    w, h = 34, 40
    dets = drawref.records([3, 17, 60], [(.9, .3, .3, .4, .5), (.5, .7, .6, .5, .3), (.3, .5, .5, .9, .9)])
    cases = []
    for fmt in ("rgb24", "yuyv"):
        def call(ctx, i, o, st, fmt=fmt):
            _, L = _lib()
            drawn = C.c_int(0)
            hipdrv.check(L.yolo2_hip_annotate_pix(i, w, h, hipdrv.PIXFMTS[fmt], dets.ctypes.data_as(C.c_void_p), len(dets), 0.24, None, 0, o,
                                                  C.byref(drawn), C.c_void_p(st)), "yolo2_hip_annotate_pix")
            return [np.array([drawn.value], dtype=np.int32)]

        def anchor(values):
            assert int(values[1][0]) == 3, "the three records were not all drawn"

        a, b = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2))
        if fmt == "yuyv":
            a, b = yuyvref.rgb_to_yuyv(a), yuyvref.rgb_to_yuyv(b)
        cases.append(Case("yolo2_hip_annotate_pix", f"{w}x{h} {fmt}", np.ascontiguousarray(a), np.ascontiguousarray(b), w * h * 3, call,
                          anchor=anchor))
    return cases


def _img(w, h, k):
    """a smooth RGB frame with some noise; k selects another one of the same size"""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 5 + 40 * k) % 256, (yy * 3 + xx) % 256, (xx + yy * 2 + 90 * k) % 256], axis=2)
    noise = np.random.default_rng(100 + k).integers(-20, 21, base.shape)
    return np.clip(base + noise, 0, 255).astype(np.uint8)


def jpeg_cases():
    hipdrv, _ = _lib()
    rng = np.random.default_rng(17)
    cases = []
    for w, h in ((17, 33), (320, 240)):
        cap = hipdrv.jpeg_bound(w, h)

        def call(ctx, i, o, st, w=w, h=h, cap=cap):
            _, L = _lib()
            size = C.c_size_t(0)
            hipdrv.check(L.yolo2_hip_jpeg_encode_rgb24(i, w, h, 80, o, cap, C.byref(size), C.c_void_p(st)), "yolo2_hip_jpeg_encode_rgb24")
            return [np.array([size.value], dtype=np.int64)]

        def view(out, host):      # (bytes behind the stream's end are not part of the result)
            return [out[:int(host[0][0])], host[0]]

        def anchor(values, w=w, h=h):
            assert values[0].tobytes() == hipdrv.write_jpg_host(_img(w, h, 0), 80), "the stream differs from the host encoder's"

        cases.append(Case("yolo2_hip_jpeg_encode_rgb24", f"{w}x{h}", _img(w, h, 0), _img(w, h, 1), cap, call, view=view, anchor=anchor))
    return cases


def absmax_case():
    hipdrv, _ = _lib()
    n = (1 << 20) + 3
    rng = np.random.default_rng(20)
    a = rng.standard_normal(n).astype(np.float32)
    b = (rng.standard_normal(n) * 3).astype(np.float32)
    a[-1] = -7.25                                     # the maximum sits in the tail behind the last full vector

    def call(ctx, i, o, st):
        m, bad = hipdrv.absmax_f32(i, n, stream=st)
        return [np.array([m], dtype=np.float32), np.array([bad], dtype=np.int64)]

    def anchor(values):
        assert values[0][0] == np.float32(np.abs(a).max()) == np.float32(7.25) and values[1][0] == 0

    return Case("yolo2_hip_absmax_f32", f"n={n}", a, b, 0, call, anchor=anchor)


def calib_case():
    def call(ctx, i, o, st):
        hipdrv, L = _lib()
        ctx.calib_reset()
        hipdrv.check(L.yolo2_hip_calib_frames(ctx._h, i, 2, C.c_void_p(st)), "yolo2_hip_calib_frames")
        s = ctx.calib_stats()
        return [s["act_absmax"], s["weight_absmax"], s["bias_absmax"], np.array([s["frames_seen"]], dtype=np.int64)]

    def anchor(values):
        assert values[3][0] == 2 and np.isfinite(values[0]).all() and (values[0] > 0).all()

    return Case("yolo2_hip_calib_frames", "batch=2", frames_for(2, 0), frames_for(2, 1), 0, call, anchor=anchor)
