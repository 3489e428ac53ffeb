"""GPU tests of the camera loop as one call: k_draw_items (through its doorway yolo2_hip_draw_items_dev) against the host twin
y2h_draw_item, which tests/test_loop_host.py pins to the host painter; yolo2_hip_loop_images_pix and its multi form against the two
calls it joins (the _pix_dets entry of the precision, then the annotate entry fed those records), which the earlier test files pin to
the compiled reference; what yolo2_hip_loop_last_info says about the bytes that moved; capacities, refusals and memory."""
import os

import numpy as np
import pytest

import orclib
from drawref import host_draw, records
from loopref import ITEM_DTYPE, draw_item
from yolo2_amd import hipdrv, synth
from yuyvref import formula, rgb_to_yuyv

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
NAMES = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
C = hipdrv.C
# thresh: at 0.1 this model leaves records on the large frames only; at 0.07 the 34x20, 8x6 and 7x9 frames have some too (counted with the
# CPU oracle), so that most frames of every set have something painted
THRESH, NMS, BATCH, CAP = 0.07, 0.45, 3, 845
BEST, APP = hipdrv.DETS_BEST_CLASS, hipdrv.DETS_APP_TAIL


# ------------------------------------------------------------------ k_draw_items

def _items_expected(dets, counts, ws, hs, thresh, labels):
    """y2h_draw_item over the records in use, frame by frame: (items per frame, unprintable per frame)"""
    n, cap = dets.shape
    items, bad = [], []
    for f in range(n):
        got, nb = [], 0
        for rec in dets[f, :min(max(int(counts[f]), 0), cap)]:
            rc, it = draw_item(rec, ws[f], hs[f], thresh, labels)
            if rc == 1:
                got.append(it)
            nb += rc == -1
        items.append(np.array(got, dtype=ITEM_DTYPE))
        bad.append(nb)
    return items, bad


def _check_items(ctx, dets, counts, ws, hs, thresh, labels, expect_bad=None):
    rc, raw, n_items, bad = hipdrv.draw_items_dev(ctx._h, dets, counts, ws, hs, thresh, labels=labels)
    want, want_bad = _items_expected(dets, counts, ws, hs, thresh, labels)
    assert raw.shape[2] == ITEM_DTYPE.itemsize
    assert [int(b) for b in bad] == want_bad
    if expect_bad is None:
        assert rc == 0, hipdrv.lib().yolo2_hip_last_error()
    else:
        assert rc == hipdrv.YOLO2_ERROR and b"frame %d " % expect_bad in hipdrv.lib().yolo2_hip_last_error()
    for f in range(len(want)):
        assert int(n_items[f]) == len(want[f]), f
        got = raw[f, :len(want[f])].reshape(-1).view(ITEM_DTYPE)
        assert got.tobytes() == want[f].tobytes(), f
    return [len(w) for w in want]


def _random_records(rng, n, frame=0):
    box = np.stack([rng.uniform(.05, 1., n), rng.uniform(-.1, 1.1, n), rng.uniform(-.1, 1.1, n), rng.uniform(0, .5, n), rng.uniform(0, .5, n)], axis=1)
    return records(rng.integers(0, 80, n), box.astype(np.float32), frame)


def _pack(per, cap):
    dets = np.zeros((len(per), cap), dtype=hipdrv.DET_DTYPE)
    for f, d in enumerate(per):
        dets[f, :len(d)] = d
    return dets


def test_items_from_device_records_equal_the_host_twin():
    ctx = hipdrv.Yolo2Hip(0)      # no weights
    rng = np.random.default_rng(3)
    nan, inf = float("nan"), float("inf")
    hand = records([0, 79, 7, 16, -1, 3, 3, 5, 5, 5, 5, 81],
                   [[.9, .5, .5, .3, .3], [.3, .1, .1, .4, .1], [.125, .5, .2, .1, .1], [.375, .2, .8, .2, .2], [.9, .5, .5, .2, .2],
                    [.24, .5, .5, .2, .2], [.625, nan, .5, .2, .2], [.875, 1e30, -1e30, inf, .2], [.99, 3., 3., .2, .2], [1.0, .5, .5, 0, 0],
                    [.2400001, .02, .02, .01, .01], [.5, .7, .3, .2, .6]])
    # three frames with 0 / 1 / 17 records, the hand-made set (ties, prob == thresh, a prob below it, a negative class), 845 records in one frame,
    # a count above the capacity, a zero count behind records that must not be used
    per = [hand[:0], hand[:1], _random_records(rng, 17, 2), hand, _random_records(rng, 845, 4), _random_records(rng, 845, 5), _random_records(rng, 9, 6)]
    dets = _pack(per, 845)
    counts = np.array([0, 1, 17, len(hand), 845, 845 + 77, 0], dtype=np.int32)
    ws, hs = [64, 1, 33, 768, 320, 97, 64], [48, 1, 17, 576, 240, 3, 48]
    for labels in (NAMES, None, ["only", None, "Three!"]):
        n = _check_items(ctx, dets, counts, ws, hs, .24, labels)
        assert n[0] == 0 and n[1] == 1 and n[6] == 0 and n[3] == len(hand) - 3 and n[4] > 600
    # a small capacity: count > cap uses cap records
    _check_items(ctx, dets[:, :5].copy(), counts, ws, hs, .24, NAMES)
    # one NaN prob (and an Inf, and 2^23) among the records to be drawn: that frame is reported, every other frame is intact, and
    # the frame's other records are drawn
    d2 = dets.copy()
    was_drawn = lambda f: [i for i in range(int(counts[f])) if dets[f, i]["prob"] > .24]
    (a,), (b, c) = was_drawn(2)[3:4], was_drawn(4)[100:300:199]
    d2[2, a]["prob"], d2[4, b]["prob"], d2[4, c]["prob"] = nan, inf, 8388608.0
    n2 = _check_items(ctx, d2, counts, ws, hs, .24, NAMES, expect_bad=2)
    assert n2[2] == n[2] - 1 and n2[4] == n[4] - 2
    # -Inf is below the threshold: not drawn, not reported
    d2 = dets.copy()
    d2[2, 4]["prob"] = -inf
    _check_items(ctx, d2, counts, ws, hs, .24, NAMES)
    L = hipdrv.lib()
    for bad_kw in (dict(n=0), dict(cap=0), dict(thresh=-1.0)):
        rc = L.yolo2_hip_draw_items_dev(ctx._h, 1, 1, bad_kw.get("n", 1), bad_kw.get("cap", 1), (C.c_int * 1)(4), (C.c_int * 1)(4),
                                        bad_kw.get("thresh", .24), None, 0, (C.c_char * 512)(), (C.c_int * 1)(), None)
        assert rc == hipdrv.YOLO2_ERROR, bad_kw
    ctx.close()


# ------------------------------------------------------------------ the loop against the two calls

def _natural(w, h):
    return np.ascontiguousarray(DOG[np.arange(h) * DOG.shape[0] // h][:, np.arange(w) * DOG.shape[1] // w])


def _frames(fmt):
    """7 frames: three chunks of 3, buffer set 0 used twice, the last chunk partial"""
    if fmt == "yuyv":
        rgb = [DOG, _natural(64, 48), _natural(34, 20), _natural(8, 6), np.ascontiguousarray(DOG[:, ::-1]), _natural(320, 240), _natural(300, 700)]
        return [rgb_to_yuyv(im) for im in rgb]
    rgb = [DOG, _natural(64, 48), _natural(34, 20), _natural(8, 6), _natural(7, 9), _natural(1, 1), np.ascontiguousarray(DOG[:, ::-1])]
    return rgb if fmt == "rgb24" else [np.ascontiguousarray(im[:, :, 1]) for im in rgb]


def _as_rgb(fmt, im):
    return formula(im) if fmt == "yuyv" else (im if fmt == "rgb24" else np.repeat(im[:, :, None], 3, axis=2))


@pytest.fixture(scope="module")
def ctx():
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    yield c
    c.close()


_two_calls = {}


def two_calls(ctx, fmt, precision, tail):
    """the route the loop replaces, once per (format, precision, tail): records from the _pix_dets entry, then both annotate entries"""
    key = (fmt, precision, tail)
    if key not in _two_calls:
        frames = _frames(fmt)
        r = hipdrv.run_images_dets(ctx._h, frames, BATCH, THRESH, NMS, cap=CAP, precision=precision, pixfmt=fmt, tail=tail)
        rgb, drawn = ctx.annotate_images(frames, r["dets"], None, BATCH, THRESH, labels=NAMES, pixfmt=fmt)
        jpg, drawn_j = ctx.annotate_images(frames, r["dets"], None, BATCH, THRESH, labels=NAMES, pixfmt=fmt, jpeg_quality=80)
        assert list(drawn) == list(drawn_j)
        print(f"two calls {key}: counts {list(r['counts'])} drawn {list(drawn)}")
        # what keeps the comparison honest: most frames have something painted
        assert sum(int(d) > 0 for d in drawn) >= 4 and int(sum(drawn)) >= 10, list(drawn)
        _two_calls[key] = (frames, r, rgb, jpg, [int(d) for d in drawn])
    return _two_calls[key]


@pytest.mark.parametrize("out", ["rgb24", "jpeg"])
@pytest.mark.parametrize("tail", ["core", "app"])
@pytest.mark.parametrize("precision", ["int16", "fp16", "fp32fast"])
@pytest.mark.parametrize("fmt", ["yuyv", "rgb24", "grey8"])
def test_loop_equals_the_two_calls(ctx, fmt, precision, tail, out):
    frames, r, rgb, jpg, drawn = two_calls(ctx, fmt, precision, tail)
    got = ctx.loop_images(frames, pixfmt=fmt, precision=precision, tail=tail, thresh=THRESH, nms=NMS, labels=NAMES,
                          jpeg_quality=80 if out == "jpeg" else None, batch=BATCH, cap=CAP)
    assert np.array_equal(got["counts"], r["counts"]) and got["final_q"] == r["final_q"]
    for f in range(len(frames)):
        assert got["dets"][f].tobytes() == r["dets"][f].tobytes(), f
        assert (got["dets"][f]["frame"] == f).all()
        if out == "jpeg":
            assert got["frames"][f] == jpg[f], f
        else:
            assert np.array_equal(got["frames"][f], rgb[f]), f
    assert [int(d) for d in got["drawn"]] == drawn
    if (precision, tail, out) == ("int16", "app", "rgb24"):      # the reference's loop itself: its tail's records through its painter
        for f in range(len(frames)):
            want, n = host_draw(_as_rgb(fmt, frames[f]), r["dets"][f], THRESH, NAMES)
            assert n == drawn[f] and np.array_equal(got["frames"][f], want), f
    # ---- what moved
    info = ctx.loop_last_info()
    pad = lambda b: (b + 255) & ~255
    chunks = [frames[k:k + BATCH] for k in range(0, len(frames), BATCH)]
    # a chunk's upload: LetterboxItem[batch] (56 bytes each), AnnoHeader (312) + AnnoFrame[batch] (40 each), the frames padded to 256
    tables = pad(BATCH * 56) + pad(312 + BATCH * 40)
    frame_h2d = sum(pad(im.nbytes) for im in frames)
    assert info["chunks"] == 3 and info["items_kernel"] == "k_draw_items"
    assert info["image_bytes_staged"] == sum(im.nbytes for im in frames)
    assert info["items_built"] == sum(drawn)
    rgb_bytes = sum(im.shape[0] * im.shape[1] * 3 for im in frames)
    if out == "rgb24":
        assert info["image_bytes_h2d"] == len(chunks) * tables + frame_h2d      # every frame went up once
        assert info["out_bytes_d2h"] == sum(pad(im.shape[0] * im.shape[1] * 3) for im in frames)
    else:      # ... plus the encoder's table behind each chunk's frames: its Tables (5216 bytes) and one JpegFrame (56) per frame of the chunk
        jtables = sum(pad(5216 + len(ck) * 56) for ck in chunks)
        assert info["image_bytes_h2d"] == len(chunks) * tables + frame_h2d + jtables
        assert info["out_bytes_d2h"] == sum(len(j) for j in jpg) + 8 * len(frames) and info["out_bytes_d2h"] < rgb_bytes


def _raw(ctx, frames, fmt, caps, out_format=1, quality=80, flags=BEST, precision=0, guard=16, multi=False, handle=None):
    return hipdrv.loop_images_raw(handle if handle is not None else ctx._h, frames, fmt, precision, flags, THRESH, NMS, BATCH, CAP, NAMES, out_format,
                                  quality, caps, multi=multi, guard=guard)


def test_one_capacity_too_small(ctx):
    frames, r, rgb, jpg, drawn = two_calls(ctx, "rgb24", "int16", "core")
    L = hipdrv.lib()
    for short, cap in ((0, len(jpg[0]) - 1), (3, 100), (6, 0)):
        caps = [len(j) + 5 for j in jpg]
        caps[short] = cap
        rc, dets, counts, q, outs, sizes, dr = _raw(ctx, frames, "rgb24", caps)
        assert rc == hipdrv.YOLO2_ERROR and b"too small for frame %d" % short in L.yolo2_hip_last_error(), short
        assert np.array_equal(counts, r["counts"]) and [int(d) for d in dr] == drawn
        for f in range(len(frames)):
            k = min(caps[f], len(jpg[f]))
            assert int(sizes[f]) == len(jpg[f]) and outs[f][:k].tobytes() == jpg[f][:k] and (outs[f][k:] == 0xA5).all(), (short, f)
            assert dets[f, :len(r["dets"][f])].tobytes() == r["dets"][f].tobytes()
    # RGB24: a capacity below w * h * 3 is refused before anything is launched
    caps = [im.shape[0] * im.shape[1] * 3 for im in frames]
    caps[4] -= 1
    rc, dets, counts, q, outs, sizes, dr = _raw(ctx, frames, "rgb24", caps, out_format=0)
    assert rc == hipdrv.YOLO2_ERROR and b"too small for frame 4" in L.yolo2_hip_last_error()
    assert all((o == 0xA5).all() for o in outs) and not counts.any() and not sizes.any()


def test_refusals_launch_nothing_and_memory_balances():
    frames = _frames("yuyv")[:4]
    L = hipdrv.lib()
    base = hipdrv.live_bytes()
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)      # int16 weights only
    held = hipdrv.live_bytes()
    caps = [hipdrv.jpeg_bound(im.shape[1], im.shape[0]) for im in frames]

    def refused(what, **kw):
        fr = kw.pop("frames", frames)
        rc, dets, counts, q, outs, sizes, dr = _raw(c, fr, "yuyv", kw.pop("caps", caps), **kw)
        assert rc == hipdrv.YOLO2_ERROR and what in L.yolo2_hip_last_error(), (what, L.yolo2_hip_last_error())
        assert hipdrv.live_bytes() == held, what
        assert all((o == 0xA5).all() for o in outs) and not counts.any() and not sizes.any() and not dr.any()
    refused(b"YOLO2_DETS_BEST_CLASS", flags=0)
    refused(b"YOLO2_DETS_BEST_CLASS", flags=APP)
    refused(b"fp32 weights not loaded", precision=1)
    refused(b"fp32 weights not loaded", precision=2)
    refused(b"quality 0", quality=0)
    refused(b"quality 101", quality=101)
    refused(b"precision", precision=3)
    refused(b"output format", out_format=2)
    # an odd YUYV width: the same bytes declared one pixel narrower (through the raw entry)
    n, ptrs, ws, hs, code, keep = hipdrv._image_args(frames, "yuyv")
    ws[1] -= 1
    dets = np.zeros((n, CAP), dtype=hipdrv.DET_DTYPE)
    counts, sizes, cap_arr = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.array(caps, np.uint64)
    outs = [np.full(k, 0xA5, dtype=np.uint8) for k in caps]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [c._h, 0, ptrs, ws, hs, code, n, BATCH, THRESH, NMS, BEST, vp(dets), CAP, vp(counts), None, None, 0, 1, 80, optrs, vp(cap_arr), vp(sizes), None]
    assert L.yolo2_hip_loop_images_pix(*args) == hipdrv.YOLO2_ERROR and b"even width" in L.yolo2_hip_last_error()
    ws[1] += 1
    for k, what in ((2, b"null"), (11, b"null"), (13, b"null"), (19, b"null"), (20, b"null"), (21, b"null")):
        a = list(args)
        a[k] = None
        assert L.yolo2_hip_loop_images_pix(*a) == hipdrv.YOLO2_ERROR and what in L.yolo2_hip_last_error(), k
    for k, v in ((5, 7), (6, 0), (7, 1025), (7, 0), (8, -0.5), (12, 0)):
        a = list(args)
        a[k] = v
        assert L.yolo2_hip_loop_images_pix(*a) == hipdrv.YOLO2_ERROR, (k, v)
    assert hipdrv.live_bytes() == held and all((o == 0xA5).all() for o in outs)
    # and the call itself works on this context, then everything is given back
    assert L.yolo2_hip_loop_images_pix(*args) == 0, L.yolo2_hip_last_error()
    assert hipdrv.live_bytes() != held and counts.any() and sizes.all()
    c.close()
    assert hipdrv.live_bytes() == base


@pytest.mark.parametrize("precision", ["int16", "fp16"])
def test_multi_entry_equals_the_single_context(ctx, precision):
    frames, r, rgb, jpg, drawn = two_calls(ctx, "yuyv", precision, "app")
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    m = hipdrv.Yolo2HipMulti([0, 0])
    if precision == "int16":
        m.load_model(model)
    else:
        m.load_model_fp32(model)
    for quality, want in ((None, rgb), (80, jpg)):
        got = m.loop_images(frames, batch_per_device=2, pixfmt="yuyv", precision=precision, tail="app", thresh=THRESH, nms=NMS, labels=NAMES,
                            jpeg_quality=quality, cap=CAP)
        assert np.array_equal(got["counts"], r["counts"]) and got["final_q"] == r["final_q"] and [int(d) for d in got["drawn"]] == drawn
        for f in range(len(frames)):
            assert got["dets"][f].tobytes() == r["dets"][f].tobytes() and (got["dets"][f]["frame"] == f).all(), f
            assert got["frames"][f] == want[f] if quality else np.array_equal(got["frames"][f], want[f]), f
    m.close()


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    import subprocess
    cli = os.path.join(PKG, "yolov2_detect")
    return subprocess.run([cli, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_loop_gpu_writes_what_the_two_calls_write(tmp_path):
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    images = [np.ascontiguousarray(DOG[::2, ::2]), np.ascontiguousarray(DOG[100:340, 200:520]), np.ascontiguousarray(DOG[::4, ::3]),
              np.ascontiguousarray(DOG[::3, ::3][:, ::-1]), _natural(34, 20)]
    (tmp_path / "in").mkdir()
    for k, im in enumerate(images):
        (tmp_path / "in" / f"im{k}.ppm").write_bytes(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
    common = ["--weights", str(tmp_path / "weights"), "--batch", "2", "--chunk-batches", "1", "--thresh", "0.1", "--input-dir", str(tmp_path / "in"),
              "--annotate-gpu"]
    files = 0
    for k, extra in enumerate((["--annotated-format", "jpg"], ["--annotated-format", "ppm"], ["--tail", "app"],
                               ["--tail", "app", "--precision", "fp16", "--annotated-format", "jpg"])):
        outs = []
        for loop in (False, True):
            d = tmp_path / f"out{k}{int(loop)}"
            res = _cli(common + extra + ["--save-annotated-dir", str(d), "--jsonl", str(d) + ".jsonl"] + (["--loop-gpu"] if loop else []), tmp_path)
            assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
            dets = [ln for ln in res.stdout.splitlines() if ln.startswith("  ") and "%" in ln]
            outs.append((sorted(os.listdir(d)), [(d / n).read_bytes() for n in sorted(os.listdir(d))], open(str(d) + ".jsonl").read(), dets))
        assert outs[0][0] == outs[1][0] and len(outs[0][0]) == len(images)
        assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2] and outs[0][3] == outs[1][3] and len(outs[0][3]) > 4
        files += len(outs[0][0])
    assert files == 4 * len(images)
