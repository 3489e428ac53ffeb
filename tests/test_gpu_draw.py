"""GPU tests of the annotated frame: yolo2_hip_annotate_pix / _annotate_images_pix_host / _multi_annotate_images_pix_host and the
CLI's --annotate-gpu paint exactly what the reference's yolo2_draw_detections_rgb24 paints.  The expected side is the fixture the
compiled reference made (tests/golden/draw.npz) and, at the sizes it does not hold, the host restatement y2h_draw_detections_rgb24,
which tests/test_draw_host.py pins to that fixture - never the code under test."""
import os
import subprocess

import numpy as np
import pytest

import orclib
from drawref import CASES, case, host_draw, records
from yolo2_amd import hipdrv, synth
from yuyvref import formula

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
NAMES = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
C = hipdrv.C


def _random_records(rng, n, frame=0):
    """n records all over (and partly off) the frame, every class, probabilities on both sides of 0.24"""
    box = np.stack([rng.uniform(.05, 1., n), rng.uniform(-.1, 1.1, n), rng.uniform(-.1, 1.1, n), rng.uniform(0, .5, n), rng.uniform(0, .5, n)], axis=1)
    return records(rng.integers(0, 80, n), box.astype(np.float32), frame)


@pytest.mark.parametrize("name", CASES)
def test_annotate_pix_rgb24_equals_the_reference(name):
    frame, dets, thresh, labels, expect, drawn = case(name)
    out, n = hipdrv.annotate_pix(frame, dets, "rgb24", thresh, labels)
    assert n == drawn
    assert np.array_equal(out, expect)


@pytest.mark.parametrize("w,h", [(2, 1), (6, 5), (34, 40)])
def test_annotate_pix_yuyv_and_grey_equal_the_restatement_on_the_converted_frame(w, h):
    rng = np.random.default_rng(w * 100 + h)
    dets = _random_records(rng, 6)
    yuyv = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
    want, n_want = host_draw(formula(yuyv), dets, .24, NAMES)
    got, n = hipdrv.annotate_pix(yuyv, dets, "yuyv", .24, NAMES)
    assert n == n_want > 0 and np.array_equal(got, want)
    for gw in (w, w + 1):      # grey frames may have an odd width
        grey = rng.integers(0, 256, (h, gw), dtype=np.uint8)
        want, n_want = host_draw(np.repeat(grey[:, :, None], 3, axis=2), dets, .24, None)
        got, n = hipdrv.annotate_pix(grey, dets, "grey8", .24, None)
        assert n == n_want and np.array_equal(got, want)


def test_annotate_pix_at_an_odd_output_address():
    """rgb_out_dev and an RGB24 image_dev need no alignment: the byte path gives the same frame"""
    frame, dets, thresh, labels, expect, drawn = case("main")
    L = hipdrv.lib()
    src = hipdrv.DevBuf(np.concatenate([np.zeros(1, dtype=np.uint8), frame.reshape(-1)]))
    dst = hipdrv.DevBuf(nbytes=frame.size + 8)
    lab = (C.c_char_p * len(labels))(*[s.encode() for s in labels])
    n = C.c_int(0)
    hipdrv.check(L.yolo2_hip_annotate_pix(src.addr + 1, 96, 64, 3, dets.ctypes.data_as(C.c_void_p), len(dets), thresh, lab, len(labels), dst.addr + 3,
                                          C.byref(n), None), "yolo2_hip_annotate_pix")
    out = dst.get(np.uint8, (frame.size + 8,))
    src.free()
    dst.free()
    assert n.value == drawn and np.array_equal(out[3:3 + frame.size].reshape(frame.shape), expect)
    assert not out[:3].any() and not out[3 + frame.size:].any()


def _mixed_set():
    """nine RGB frames from 1x1 to 320x240 with their records [9][845] and counts: the fixture's 845-record frame, a frame of 19
    strips with 300 records all over it, zero-record frames, a count above the capacity"""
    rng = np.random.default_rng(9)
    sizes = [(1, 1), (64, 48), (320, 240), (33, 17), (2, 2), (160, 120), (97, 3), (5, 211), (128, 96)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    many = case("many845")
    frames[1] = many[0]
    per = [_random_records(rng, k, f) for f, k in enumerate([2, 0, 300, 4, 1, 0, 3, 7, 40])]
    per[1] = many[1]
    per[8] = _random_records(rng, 845, 8)
    dets = np.zeros((9, 845), dtype=hipdrv.DET_DTYPE)
    for f, d in enumerate(per):
        dets[f, :len(d)] = d
    counts = np.array([len(d) for d in per], dtype=np.int32)
    counts[8] = 845 + 60      # more than the capacity: the 845 that are there are used
    return frames, dets, counts


def test_batched_entry_equals_the_per_frame_entry_and_the_restatement():
    frames, dets, counts = _mixed_set()
    want = [host_draw(frames[f], dets[f, :min(counts[f], 845)], .24, NAMES) for f in range(9)]
    assert want[1][1] == 845 and want[5][1] == 0 and want[2][1] > 128
    for f in (0, 1, 2, 6):
        got, n = hipdrv.annotate_pix(frames[f], dets[f, :min(counts[f], 845)], "rgb24", .24, NAMES)
        assert n == want[f][1] and np.array_equal(got, want[f][0]), f
    ctx = hipdrv.Yolo2Hip(0)      # no weights
    for batch in (1, 3, 4, 64):   # nine frames at batch 4: a ragged last chunk
        outs, drawn = ctx.annotate_images(frames, dets, counts, batch, .24, labels=NAMES)
        for f in range(9):
            assert drawn[f] == want[f][1] and np.array_equal(outs[f], want[f][0]), (batch, f)
    # YUYV and grey chunks (a call is one format), labels = NULL
    rng = np.random.default_rng(10)
    yuyv = [rng.integers(0, 256, (fr.shape[0], fr.shape[1] + (fr.shape[1] & 1), 2), dtype=np.uint8) for fr in frames]
    outs, drawn = ctx.annotate_images(yuyv, dets, counts, 4, .24, pixfmt="yuyv")
    for f in range(9):
        w_img, n = host_draw(formula(yuyv[f]), dets[f, :min(counts[f], 845)], .24, None)
        assert drawn[f] == n and np.array_equal(outs[f], w_img), f
    grey = [np.ascontiguousarray(fr[:, :, 0]) for fr in frames]
    outs, drawn = ctx.annotate_images(grey, dets, counts, 3, .24, pixfmt="grey8")
    for f in range(9):
        w_img, n = host_draw(np.repeat(grey[f][:, :, None], 3, axis=2), dets[f, :min(counts[f], 845)], .24, None)
        assert drawn[f] == n and np.array_equal(outs[f], w_img), f
    ctx.close()


@pytest.mark.parametrize("precision", ["int16", "fp16"])
def test_records_of_the_network_draw_the_restatements_frame(precision):
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    images = [DOG, np.ascontiguousarray(DOG[::3, ::2])]
    ctx = hipdrv.Yolo2Hip(0)
    if precision == "int16":
        ctx.load_model(model)
    else:
        ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    r = hipdrv.run_images_dets(ctx._h, images, 2, .05, .45, cap=845, precision=precision)
    outs, drawn = ctx.annotate_images(images, r["dets"], None, 2, .05, labels=NAMES)
    ctx.close()
    assert drawn.sum() > 4
    for f, im in enumerate(images):
        want, n = host_draw(im, r["dets"][f], .05, NAMES)
        assert drawn[f] == n == len(r["dets"][f]) and np.array_equal(outs[f], want), f


def test_multi_entry_equals_the_single_context():
    frames, dets, counts = _mixed_set()
    ctx = hipdrv.Yolo2Hip(0)
    single, drawn1 = ctx.annotate_images(frames, dets, counts, 2, .24, labels=NAMES)
    ctx.close()
    m = hipdrv.Yolo2HipMulti([0, 0])
    multi, drawn2 = m.annotate_images(frames, dets, counts, 2, .24, labels=NAMES)
    m.close()
    assert np.array_equal(drawn1, drawn2)
    for a, b in zip(single, multi):
        assert np.array_equal(a, b)


def test_bad_arguments_are_refused_nothing_is_launched_and_memory_balances():
    L = hipdrv.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    base = hipdrv.live_bytes()
    ctx = hipdrv.Yolo2Hip(0)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (12, 16, 3), dtype=np.uint8) for _ in range(2)]
    n, ptrs, ws, hs, fmt, keep = hipdrv._image_args(frames, "rgb24")
    dets = np.zeros((2, 4), dtype=hipdrv.DET_DTYPE)
    dets[:, :] = records([1, 2, 3, 4], [(.9, .5, .5, .4, .4)] * 4)
    counts = np.array([4, 2], dtype=np.int32)
    outs = [np.full((12, 16, 3), 0xA5, dtype=np.uint8) for _ in range(2)]
    optrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    bad_prob = dets.copy()
    bad_prob["prob"][1, 1] = np.inf
    nan_prob = dets.copy()
    nan_prob["prob"][0, 3] = np.nan
    odd = (C.c_int * 2)(16, 15)
    zero = (C.c_int * 2)(16, 0)
    null_img = (C.c_void_p * 2)(ptrs[0], None)
    null_out = (C.c_void_p * 2)(None, optrs[1])
    YUYV = hipdrv.PIXFMTS["yuyv"]

    def batched(p=ptrs, w=ws, h=hs, f=fmt, nn=n, batch=2, d=dets, cap=4, c=counts, thresh=.24, o=optrs, handle=None, multi=None):
        fn = L.yolo2_hip_multi_annotate_images_pix_host if multi else L.yolo2_hip_annotate_images_pix_host
        return fn(multi if multi else (ctx._h if handle is None else handle), p, w, h, f, nn, batch, vp(d) if d is not None else None, cap,
                  vp(c) if c is not None else None, thresh, None, 0, o, None)

    held = hipdrv.live_bytes()
    for kw, text in ((dict(p=None), b"null"), (dict(w=None), b"null"), (dict(d=None), b"null"), (dict(c=None), b"null"), (dict(o=None), b"null"),
                     (dict(p=null_img), b"null image or output 1"), (dict(o=null_out), b"null image or output 0"),
                     (dict(w=odd, f=YUYV), b"even width, not 15"), (dict(f=2), b"unknown pixel format"), (dict(thresh=-.5), b"thresh"),
                     (dict(thresh=float("nan")), b"thresh"), (dict(w=zero), b"bad frame size"), (dict(nn=0), b"image count"),
                     (dict(batch=0), b"batch"), (dict(cap=0), b"capacity"), (dict(d=bad_prob), b"record 1 of frame 1 has a non-finite prob"),
                     (dict(d=nan_prob), b"record 3 of frame 0 has a non-finite prob")):
        assert batched(**kw) == hipdrv.YOLO2_ERROR, kw
        assert text in L.yolo2_hip_last_error(), (kw, L.yolo2_hip_last_error())
        assert hipdrv.live_bytes() == held, kw
    # a non-finite prob beyond the records that are used is not looked at
    beyond = dets.copy()
    beyond["prob"][1, 3] = np.nan
    assert batched(d=beyond) == 0 and not (outs[0] == 0xA5).all()
    for o in outs:
        o[:] = 0xA5
    m = hipdrv.Yolo2HipMulti([0, 0])
    for kw, text in ((dict(p=None), b"null"), (dict(w=odd, f=YUYV), b"even width, not 15"), (dict(d=bad_prob), b"non-finite prob"), (dict(nn=-1), b"image count")):
        assert batched(multi=m._m, **kw) == hipdrv.YOLO2_ERROR, kw
        assert text in L.yolo2_hip_last_error(), (kw, L.yolo2_hip_last_error())
    m.close()
    assert all((o == 0xA5).all() for o in outs)      # no refused call wrote a frame
    # the single-image entry
    src, dst = hipdrv.DevBuf(frames[0]), hipdrv.DevBuf(np.full(12 * 16 * 3, 0xA5, dtype=np.uint8))
    one = np.ascontiguousarray(dets[0])
    held = hipdrv.live_bytes()

    def single(image=None, w=16, h=12, f=3, d=one, nd=4, thresh=.24, out=None):
        return L.yolo2_hip_annotate_pix(src.addr if image is None else image, w, h, f, vp(d) if d is not None else None, nd, thresh, None, 0,
                                        dst.addr if out is None else out, None, None)

    for kw, text in ((dict(image=0), b"null"), (dict(out=0), b"null"), (dict(d=None), b"null records"), (dict(nd=-1), b"null records"),
                     (dict(w=15, f=YUYV), b"even width, not 15"), (dict(f=0), b"unknown pixel format"), (dict(thresh=-1.), b"thresh"),
                     (dict(h=0), b"bad frame size"), (dict(w=-3), b"bad frame size"), (dict(d=np.ascontiguousarray(bad_prob[1])), b"non-finite prob"),
                     (dict(image=src.addr + 2, w=8, f=YUYV), b"4-byte boundary")):
        assert single(**kw) == hipdrv.YOLO2_ERROR, kw
        assert text in L.yolo2_hip_last_error(), (kw, L.yolo2_hip_last_error())
        assert hipdrv.live_bytes() == held, kw
    assert (dst.get(np.uint8, (12 * 16 * 3,)) == 0xA5).all()
    assert single() == 0 and hipdrv.live_bytes() == held
    src.free()
    dst.free()
    # the context still works, and gives everything back when it is closed
    good, drawn = ctx.annotate_images(frames, dets, counts, 1, .24)
    assert drawn.tolist() == [4, 2] and np.array_equal(good[1], host_draw(frames[1], dets[1, :2], .24, None)[0])
    assert hipdrv.live_bytes() != base
    ctx.close()
    assert hipdrv.live_bytes() == base


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def _read_ppm(path):
    data = path.read_bytes()
    head = data.split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = (int(v) for v in head[1].split())
    return np.frombuffer(head[3], dtype=np.uint8).reshape(h, w, 3)


def _old_writer(rgb, dets):
    """the writer's own frame without --annotate-gpu (host/yolov2_detect.cpp): bytes / 255 as floats, y2h::draw_box per record in its hue
    colour, save_ppm's 255 * v truncated"""
    h, w = rgb.shape[:2]
    im = rgb.astype(np.float32) / np.float32(255.)
    thick = max(1, int(h * .006))
    for d in dets:
        hue = np.float32((int(d["cls"]) * 123457) % 80) / np.float32(80)
        col = np.array([hue, np.float32(1.) - hue, np.float32(.5)], dtype=np.float32)
        x, y, bw, bh = (np.float32(d[k]) for k in ("x", "y", "w", "h"))
        x1, y1 = int((float(x) - float(bw) / 2.) * w), int((float(y) - float(bh) / 2.) * h)
        x2, y2 = int((float(x) + float(bw) / 2.) * w), int((float(y) + float(bh) / 2.) * h)
        for t in range(thick):
            a1, a2 = min(max(x1 + t, 0), w - 1), min(max(x2 - t, 0), w - 1)
            b1, b2 = min(max(y1 + t, 0), h - 1), min(max(y2 - t, 0), h - 1)
            if a1 <= a2:
                im[b1, a1:a2 + 1] = col
                im[b2, a1:a2 + 1] = col
            if b1 <= b2:
                im[b1:b2 + 1, a1] = col
                im[b1:b2 + 1, a2] = col
    return (np.float32(255) * np.clip(im, 0, 1)).astype(np.uint8)


def test_cli_annotate_gpu_writes_the_entrys_frames(tmp_path):
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    images = [np.ascontiguousarray(DOG[::2, ::2]), np.ascontiguousarray(DOG[100:340, 200:520]), np.ascontiguousarray(DOG[::4, ::3]),
              np.ascontiguousarray(DOG[::3, ::3][:, ::-1])]
    lines = []
    for k, im in enumerate(images):
        p = tmp_path / f"im{k}.ppm"
        p.write_bytes(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
        lines.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.1", "--input-list", str(tmp_path / "list.txt")]
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(model)
    r = hipdrv.run_images_dets(ctx._h, images, 3, .1, .45, cap=845)
    want, drawn = ctx.annotate_images(images, r["dets"], None, 3, .1, labels=NAMES)
    ctx.close()
    assert drawn.sum() > 4
    res = _cli(common + ["--annotate-gpu", "--save-annotated-dir", str(tmp_path / "gpu")], tmp_path)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    res_old = _cli(common + ["--save-annotated-dir", str(tmp_path / "host")], tmp_path)
    assert res_old.returncode == 0, res_old.stdout[-2000:] + res_old.stderr[-2000:]
    for f, im in enumerate(images):
        assert np.array_equal(_read_ppm(tmp_path / "gpu" / f"frame_{f + 1:06d}.ppm"), want[f]), f
        assert np.array_equal(want[f], host_draw(im, r["dets"][f], .1, NAMES)[0]), f
        assert np.array_equal(_read_ppm(tmp_path / "host" / f"frame_{f + 1:06d}.ppm"), _old_writer(im, r["dets"][f])), f
    res = _cli(common + ["--post", "host", "--annotate-gpu", "--save-annotated-dir", str(tmp_path / "x")], tmp_path)
    assert res.returncode != 0 and "--annotate-gpu paints the records of --post gpu" in res.stdout + res.stderr
