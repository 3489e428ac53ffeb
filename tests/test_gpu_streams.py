"""The caller-stream contract of every entry of include/yolo2_hip.h that takes a `void *stream`, on streams that are not the null
stream (harness: tests/streamref.py).  The expected side is never the call under test: it is the same entry on the null stream of a
context of its own (the routes the rest of the suite pins), computed before the side-stream work and followed by a device
synchronise, and frame 0 is anchored to the fixtures of tests/golden on top.  Equality is bitwise everywhere.

  A  late input, early clobber: every entry, at the shapes that reach each launch path
  B  back to back: two calls with different buffers and a third that reuses the first's, behind one delay, no host sync between
  C  two contexts on two streams, calls interleaved from one host thread
  D  batch changes on a live stream, on a context whose first run ever is on a side stream
  E  per-layer profiling on a side stream
  negative control: scenario A with the call on ANOTHER stream than the one that carries the late input must come out different

YOLO2_STREAM_LOG=<file> collects one line per case: entry, shape, scenario, t_enqueue, the delay's event time, equal / differ."""
import numpy as np
import pytest

import streamref as sr              # (imports torch before anything loads the library: see there)
import torch
import drawref
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu

INCONCLUSIVE = "inconclusive: delay too short (it had run out when the call returned)"

# scenario A: (entry without its prefix, shape label); the Case objects are built on first use
A_IDS = ([("run_batch_int16", f"batch={b}") for b in (1, 2, 16)] +
         [("run_batch_fp16", f"batch={b}") for b in (2, 64)] +
         [("run_batch_f32tol", f"batch={b}") for b in (2, 64)] +
         [("run_batch_fp32", "batch=2")] +
         [("run_batch_int8", f"batch={b}") for b in (2, 5)] +
         [("letterbox_u8", s) for s in ("57x41 rgb", "33x80 grey")] +
         [("letterbox_pix", s) for s in ("57x41 rgb24", "33x80 grey8", "2x2 yuyv", "640x480 yuyv")] +
         [("postprocess_" + s, "batch=3") for s in ("int16", "f32", "int16_app", "f32_app")] +
         [("annotate_pix", s) for s in ("34x40 rgb24", "34x40 yuyv")] +
         [("jpeg_encode_rgb24", s) for s in ("17x33", "320x240")] +
         [("absmax_f32", f"n={(1 << 20) + 3}"), ("calib_frames", "batch=2")])
LANES = {("int16", 16): 2, ("fp16", 64): 2, ("f32tol", 64): 2}      # the batches that are there for the two-lane launch path

_cases = {}


def net_case(prec, batch, k=0):
    return sr.net_case(prec, batch, k, lanes=LANES.get((prec, batch)))


def a_case(entry, label):
    if not _cases:
        for prec, name in sr.NET_ENTRIES.items():
            for b in (1, 2, 5, 16, 64):
                if (name[len("yolo2_hip_"):], f"batch={b}") in A_IDS:
                    _cases[(name, f"batch={b}")] = net_case(prec, b)
        for c in sr.letterbox_cases() + sr.tail_cases() + sr.annotate_cases() + sr.jpeg_cases() + [sr.absmax_case(), sr.calib_case()]:
            _cases[c.key] = c
    return _cases[("yolo2_hip_" + entry, label)]


class World:
    pass


@pytest.fixture(scope="module")
def world():
    """SynthModel(seed=1) as int16, fp32 and (calibrated here from four pool frames) int8 weights on three contexts: `ref` only ever
    runs on the null stream and gives the expected values, `t1` and `t2` only ever run on side streams."""
    assert hipdrv.lib().yolo2_hip_device_count() >= 1, "no GPU visible: these tests must run on the GPU box"
    w = World()
    w.model = synth.SynthModel(seed=1)

    def make(cal=None):
        ctx = hipdrv.Yolo2Hip(0)
        ctx.load_model(w.model)
        ctx.load_weights_fp32(w.model.weights_f32(), w.model.bias_f32())
        if cal is not None:
            ctx.load_model(cal)
        return ctx
    w.make = make
    w.ref = make()
    w.cal = w.ref.calibrate_int8(frames=sr.frame_pool()[:4], batch=4)
    w.ref.load_model(w.cal)
    w.t1, w.t2 = make(w.cal), make(w.cal)
    yield w
    for c in (w.ref, w.t1, w.t2):
        c.close()


def test_every_stream_taking_entry_has_a_case():
    assert {"yolo2_hip_" + e for e, _ in A_IDS} == set(sr.ENTRIES)


# ------------------------------------------------------------------ A

@pytest.mark.parametrize("entry,label", A_IDS, ids=[f"{e}-{s.replace(' ', '_')}" for e, s in A_IDS])
def test_a_late_input_early_clobber(world, entry, label):
    case = a_case(entry, label)
    equal, done = sr.scenario_a(case, world.t1, world.ref)
    if case.kind == "enqueue":
        assert not done, INCONCLUSIVE
    else:
        assert done, f"{case.entry} returned before the work in front of it on its stream had finished: it did not synchronise the stream"
    assert equal, f"{case.entry} {label}: the result on a side stream differs from the null stream's"


# ------------------------------------------------------------------ negative control

@pytest.mark.parametrize("entry,label,where", [("run_batch_int16", "batch=2", "side"),
                                                       ("letterbox_u8", "57x41 rgb", "side"),
                                                       ("run_batch_int16", "batch=2", "null")],
                         ids=["int16-other_side_stream", "letterbox_u8-other_side_stream", "int16-null_stream"])
def test_negative_control_call_on_another_stream_differs(world, entry, label, where):
    """Scenario A with the entry handed ANOTHER stream than the one that carries the late input (a second side stream; and, for the
    mistake the module is mostly about, the null stream): nothing orders the call behind the input then, so it must read the poison -
    valid memory holding other valid frames - and the result MUST differ.  If it comes out equal, streams serialise implicitly on
    this machine or the delay is too short to expose a misordering, and every pass above means nothing."""
    case = a_case(entry, label)
    other = sr.side_stream() if where == "side" else torch.cuda.default_stream()
    equal, done = sr.scenario_a(case, world.t1, world.ref, call_stream=other, scenario=f"negative-control({where})")
    assert not done, INCONCLUSIVE
    assert not equal, "the harness is toothless here: a call that nothing orders behind its input still saw the input"


# ------------------------------------------------------------------ B

B_IDS = [("int16", 1), ("int16", 2), ("int16", 16), ("fp16", 2), ("fp16", 64), ("f32tol", 2), ("fp32", 2), ("int8", 2)]


@pytest.mark.parametrize("prec,batch", B_IDS, ids=[f"{p}-batch={b}" for p, b in B_IDS])
def test_b_back_to_back(world, prec, batch):
    """Behind one delay on one stream and one context: call 1 (buffers 1), call 2 (other input, buffers 2), then - the first output
    drained and the first input replaced on the stream - call 3 on buffers 1 again; no host sync anywhere.  Context scratch, lane
    events and internal tensors are reused by a call enqueued before the one in front of it has run; all three must be right."""
    cases = [net_case(prec, batch, k) for k in range(3)]
    exps = [sr.expected(c, world.ref) for c in cases]
    ctx, s = world.t1, sr.side_stream()
    call = lambda i, o: cases[0].call(ctx, sr.ptr(i), sr.ptr(o), s.cuda_stream)
    true = [sr.dev(c.true) for c in cases]
    poison = sr.dev(cases[2].poison)                             # (input number 3: none of the three)
    in1, in2 = poison.clone(), poison.clone()
    (out1, p1), (out2, p2), (_, p3) = (sr.out_bufs(cases[0].out_nbytes) for _ in range(3))
    call(in1, out1)                                              # warm at this batch
    torch.cuda.synchronize()
    out1.fill_(sr.FILL)
    torch.cuda.synchronize()
    t_enq = sum(e.t_enqueue for e in exps)
    e0, e1 = sr.delay().enqueue(s, sr.Delay.length_ms(t_enq, sum(e.t_device for e in exps)))
    with torch.cuda.stream(s):
        in1.copy_(true[0], non_blocking=True)
        in2.copy_(true[1], non_blocking=True)
    host = [call(in1, out1), call(in2, out2)]
    with torch.cuda.stream(s):
        p1.copy_(out1, non_blocking=True)
        in1.copy_(true[2], non_blocking=True)
    host.append(call(in1, out1))
    done = e1.query()
    sr.drain_and_clobber(s, out2, p2, in2, poison)
    sr.drain_and_clobber(s, out1, p3, in1, poison)
    s.synchronize()
    cases[0].check(ctx)
    got = [c.view(p.numpy(), h) for c, p, h in zip(cases, (p1, p2, p3), host)]
    equal = [sr.same(g, e.values) for g, e in zip(got, exps)]
    sr.log(cases[0].entry, f"batch={batch}", "B", t_enq, e0.elapsed_time(e1), "equal" if all(equal) else f"differ{equal}",
           f"delay_done_on_return={int(done)}")
    assert not done, INCONCLUSIVE
    assert all(equal), f"calls 1..3 equal to the null stream's: {equal}"


# ------------------------------------------------------------------ C

@pytest.mark.parametrize("pa,pb", [("int16", "int16"), ("fp16", "int16"), ("int8", "fp16")], ids=lambda p: p)
def test_c_two_contexts_two_streams(world, pa, pb):
    """Two contexts, each behind its own delay on its own stream, two calls each, enqueued A B A B from one host thread: every result
    equals the solo result of the same input (state shared between contexts - file-scope scratch, tables - would mix them)."""
    sides = []
    for ctx, prec, k0 in ((world.t1, pa, 0), (world.t2, pb, 1)):
        cases = [net_case(prec, 2, k0 + j) for j in range(2)]
        exps = [sr.expected(c, world.ref) for c in cases]
        sides.append(dict(ctx=ctx, cases=cases, exps=exps, s=sr.side_stream(avoid=[d["s"] for d in sides]), true=[sr.dev(c.true) for c in cases],
                          poison=sr.dev(cases[1].poison), bufs=[sr.out_bufs(c.out_nbytes) for c in cases]))
    for d in sides:
        d["ins"] = [d["poison"].clone() for _ in range(2)]
        d["cases"][0].call(d["ctx"], sr.ptr(d["ins"][0]), sr.ptr(d["bufs"][0][0]), d["s"].cuda_stream)      # warm
        torch.cuda.synchronize()
        d["bufs"][0][0].fill_(sr.FILL)
    torch.cuda.synchronize()
    t_enq = sum(e.t_enqueue for d in sides for e in d["exps"])
    ms = sr.Delay.length_ms(t_enq, sum(e.t_device for d in sides for e in d["exps"]))
    for d in sides:
        d["ev"] = sr.delay().enqueue(d["s"], ms)
        with torch.cuda.stream(d["s"]):
            for j in range(2):
                d["ins"][j].copy_(d["true"][j], non_blocking=True)
    host = {}
    for j in range(2):
        for n, d in enumerate(sides):
            host[n, j] = d["cases"][j].call(d["ctx"], sr.ptr(d["ins"][j]), sr.ptr(d["bufs"][j][0]), d["s"].cuda_stream)
    done = [d["ev"][1].query() for d in sides]
    for d in sides:
        for j in range(2):
            sr.drain_and_clobber(d["s"], d["bufs"][j][0], d["bufs"][j][1], d["ins"][j], d["poison"])
    for d in sides:
        d["s"].synchronize()
    equal = [sr.same(d["cases"][j].view(d["bufs"][j][1].numpy(), host[n, j]), d["exps"][j].values) for n, d in enumerate(sides) for j in range(2)]
    sr.log(f"{sides[0]['cases'][0].entry}+{sides[1]['cases'][0].entry}", "batch=2", "C", t_enq, min(d["ev"][0].elapsed_time(d["ev"][1]) for d in sides),
           "equal" if all(equal) else f"differ{equal}", f"delay_done_on_return={[int(x) for x in done]}")
    assert not any(done), INCONCLUSIVE
    assert all(equal), f"(context, call) results equal to the solo ones: {equal}"


# ------------------------------------------------------------------ D

D_IDS = [("int16", (2, 16, 1, 2)), ("fp16", (2, 64, 2)), ("f32tol", (2, 64, 2)), ("fp32", (2, 5, 2)), ("int8", (2, 5, 2))]


@pytest.mark.parametrize("prec,batches", D_IDS, ids=[p for p, _ in D_IDS])
def test_d_batch_changes_on_a_live_stream(world, prec, batches):
    """A fresh context whose first run ever, and every run after it, is on a side stream, the batch changing from call to call with no
    host sync by the test: the tensors a batch change allocates (their zero fill is the conv padding) and the planning of a first
    call must be ordered with the caller's stream by the library itself."""
    cases = [net_case(prec, b, k) for k, b in enumerate(batches)]
    exps = [sr.expected(c, world.ref) for c in cases]
    torch.cuda.synchronize()
    # Best effort: memory that held 0xFF is handed back to the driver, so that the new context's allocations may recycle non-zero
    # bytes and a missing wait for a zero fill shows.  Nothing guarantees that the driver does not clear what it hands out.
    hipdrv.DevBuf(nbytes=384 << 20, fill=0xFF).free()
    ctx = hipdrv.Yolo2Hip(0)
    try:
        if prec == "int16":
            ctx.load_model(world.model)
        else:
            ctx.load_weights_fp32(world.model.weights_f32(), world.model.bias_f32())
            if prec == "int8":
                ctx.load_model(world.cal)
        s = sr.side_stream()
        true, poison = [sr.dev(c.true) for c in cases], [sr.dev(c.poison) for c in cases]
        ins = [p.clone() for p in poison]
        bufs = [sr.out_bufs(c.out_nbytes) for c in cases]
        torch.cuda.synchronize()
        t_enq = exps[0].t_enqueue
        e0, e1 = sr.delay().enqueue(s, sr.Delay.length_ms(t_enq, exps[0].t_device))
        host = []
        for n, c in enumerate(cases):
            with torch.cuda.stream(s):
                ins[n].copy_(true[n], non_blocking=True)
            host.append(c.call(ctx, sr.ptr(ins[n]), sr.ptr(bufs[n][0]), s.cuda_stream))
            c.check(ctx)
            sr.drain_and_clobber(s, bufs[n][0], bufs[n][1], ins[n], poison[n])
        s.synchronize()
        equal = [sr.same(c.view(b[1].numpy(), h), e.values) for c, b, h, e in zip(cases, bufs, host, exps)]
        sr.log(cases[0].entry, "batch=" + ">".join(str(b) for b in batches), "D", t_enq, e0.elapsed_time(e1), "equal" if all(equal) else f"differ{equal}")
        assert all(equal), f"batches {batches}: equal to the null stream's: {equal}"
    finally:
        torch.cuda.synchronize()
        ctx.close()


# ------------------------------------------------------------------ E

@pytest.mark.parametrize("prec", ["int16", "fp16"])
def test_e_profiling_on_a_side_stream(world, prec):
    """With per-layer profiling on, two runs on a side stream behind a delay: the layer times come from events recorded on that stream
    (finite, non-negative, not all zero) and the results do not change."""
    cases = [net_case(prec, 2, k) for k in range(2)]
    exps = [sr.expected(c, world.ref) for c in cases]
    ctx, s = world.t1, sr.side_stream()
    true, poison = [sr.dev(c.true) for c in cases], sr.dev(cases[1].poison)
    ins = [poison.clone() for _ in cases]
    bufs = [sr.out_bufs(c.out_nbytes) for c in cases]
    cases[0].call(ctx, sr.ptr(ins[0]), sr.ptr(bufs[0][0]), s.cuda_stream)      # warm
    torch.cuda.synchronize()
    bufs[0][0].fill_(sr.FILL)
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    try:
        t_enq = sum(e.t_enqueue for e in exps)
        e0, e1 = sr.delay().enqueue(s, sr.Delay.length_ms(t_enq, sum(e.t_device for e in exps)))
        host = []
        for n, c in enumerate(cases):
            with torch.cuda.stream(s):
                ins[n].copy_(true[n], non_blocking=True)
            host.append(c.call(ctx, sr.ptr(ins[n]), sr.ptr(bufs[n][0]), s.cuda_stream))
        done = e1.query()
        for n in range(2):
            sr.drain_and_clobber(s, bufs[n][0], bufs[n][1], ins[n], poison)
        s.synchronize()
        ms = ctx.layer_times_ms()
    finally:
        ctx.set_profiling(False)
    equal = [sr.same(c.view(b[1].numpy(), h), e.values) for c, b, h, e in zip(cases, bufs, host, exps)]
    sr.log(cases[0].entry, "batch=2", "E", t_enq, e0.elapsed_time(e1), "equal" if all(equal) else f"differ{equal}",
           f"delay_done_on_return={int(done)} layer_ms_sum={float(ms.sum()):.4f}")
    assert not done, INCONCLUSIVE
    assert np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0, ms
    # (the delay is no shorter than the two runs' device time, and an event recorded on another stream than the launches' would put the
    # delay into layer 0's time)
    assert ms.sum() < e0.elapsed_time(e1), f"layer times of {ms.sum()} ms hold the delay in front of the runs: events on another stream"
    assert all(equal), f"profiled runs equal to the null stream's: {equal}"


# ------------------------------------------------------------------ the Python wrappers

def test_wrappers_pass_their_stream_through(world):
    """hipdrv's host-array wrappers of the stream-taking entries on a side stream: what they return is what they return on the null
    stream (letterbox_u8 / letterbox_pix synchronise the stream themselves before they copy the frame back)."""
    case = a_case("letterbox_u8", "57x41 rgb")
    img = case.true
    s = sr.side_stream().cuda_stream
    assert np.array_equal(hipdrv.letterbox_u8(img, 96, 96, stream=s), hipdrv.letterbox_u8(img, 96, 96))
    assert np.array_equal(hipdrv.letterbox_pix(img, "rgb24", 96, 96, stream=s), hipdrv.letterbox_u8(img, 96, 96))
    rgb = a_case("annotate_pix", "34x40 rgb24").true
    recs = drawref.records([3], [(.9, .5, .5, .4, .4)])
    a, b = hipdrv.annotate_pix(rgb, recs, "rgb24", stream=s), hipdrv.annotate_pix(rgb, recs, "rgb24")
    assert a[1] == b[1] == 1 and np.array_equal(a[0], b[0])
    assert hipdrv.jpeg_encode(rgb, 80, stream=s) == hipdrv.jpeg_encode(rgb, 80) == hipdrv.write_jpg_host(rgb, 80)
    stats = []
    for st in (0, s):
        world.t2.calib_reset()
        world.t2.calib_frames(sr.frames_for(1), stream=st)
        stats.append(world.t2.calib_stats())
    assert stats[0]["frames_seen"] == stats[1]["frames_seen"] == 1 and np.array_equal(stats[0]["act_absmax"], stats[1]["act_absmax"])
