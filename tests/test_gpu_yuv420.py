"""GPU tests of the planar YUV 4:2:0 formats: NV12 and I420 frames through every _pix entry (letterbox, int16 / fp16 / split-fp16 /
int8 region tensors, detection records, the painter, annotated JPEG, the loop, a multi context, the CLI) are bit-identical to the
RGB24 entries fed the conversion of the same frames.  The expected side is always an RGB24 entry on yuv420ref.to_rgb() =
yuyvref.formula(to_yuyv(frame)), which tests/test_yuyv_host.py pins to the compiled reference - never the code under test.

The frame set is the issue's.  Two of its frames, 2 x 1000 and 1000 x 2, fit the 416 x 416 canvas with (2 * 416) / 1000 = 0 pixels
the short way, not 1 as the issue says: the RGB24 entry refuses them ("aspect too extreme"), and so must the new formats, with the
same message.  4 x 1000 and 1000 x 4 (fitted size 1 pixel) are added to the set so that the case the issue meant is run as well."""
import json
import os
import subprocess

import numpy as np
import pytest

import orclib
import yuv420ref
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
NAMES = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
FORMATS = yuv420ref.FORMATS
C = hipdrv.C
THRESH, NMS, BATCH, CAP = 0.07, 0.45, 3, 845
TOO_NARROW = ((2, 1000), (1000, 2))


def _natural(w, h, fmt):
    """the dog picture resampled to w x h (nearest)"""
    ys, xs = np.arange(h) * DOG.shape[0] // h, np.arange(w) * DOG.shape[1] // w
    return yuv420ref.from_rgb(DOG[ys][:, xs], fmt)


def _random(w, h, fmt):
    return yuv420ref.random_frame(np.random.default_rng(w * 10007 + h), w, h, fmt)


_sets = {}


def frame_set(fmt):
    """the issue's frames that can be letterboxed, the same pictures in either format: random 2 x 2, 6 x 6 (I420 chroma rows of 3 bytes),
    4 x 1000 and 1000 x 4 (fitted size 1 pixel), 34 x 18; natural 640 x 480, 300 x 700, 1280 x 720"""
    if fmt not in _sets:
        _sets[fmt] = [_random(2, 2, fmt), _random(6, 6, fmt), _random(4, 1000, fmt), _random(1000, 4, fmt), _random(34, 18, fmt),
                      _natural(640, 480, fmt), _natural(300, 700, fmt), _natural(1280, 720, fmt)]
    return _sets[fmt]


def seven(frames):
    """batch 3 over 7 frames: a ragged last chunk, mixed sizes in every chunk"""
    return [frames[k] for k in (5, 0, 2, 6, 1, 3, 7)]


_rgb = []


def rgb_set():
    """the conversion of the set: the expected side's input.  Computed once, from the NV12 frames; the I420 frames hold the same pictures."""
    if not _rgb:
        _rgb.extend(yuv420ref.to_rgb(f, "nv12") for f in frame_set("nv12"))
        for a, f in zip(_rgb, frame_set("i420")):
            assert np.array_equal(a, yuv420ref.to_rgb(f, "i420"))
    return _rgb


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def model():
    return synth.SynthModel(seed=1, obj_bias=2.0)


@pytest.fixture(scope="module")
def ctx(model):
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx8(model):
    """the int8 pass, calibrated as tests/test_gpu_i8_images.py does"""
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    c.load_model(c.calibrate_int8(frames=synth.frames(40, 4), batch=4))
    yield c
    c.close()


_want = {}


def want(key, make):
    """an RGB24 entry's result, computed once and shared by both formats' tests"""
    if key not in _want:
        _want[key] = make()
    return _want[key]


# ------------------------------------------------------------------ letterbox

@pytest.mark.parametrize("fmt", FORMATS)
def test_letterbox_pix_bit_identical_to_letterbox_u8_of_the_conversion(fmt):
    for k, (frame, rgb) in enumerate(zip(frame_set(fmt), rgb_set())):
        expect = want(("letterbox", k), lambda: hipdrv.letterbox_u8(rgb))
        assert _same_bits(hipdrv.letterbox_pix(frame, fmt), expect), (fmt, frame.shape)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", TOO_NARROW)
def test_frames_that_fit_with_no_pixel_are_refused_like_their_conversion(fmt, w, h):
    frame = _random(w, h, fmt)
    with pytest.raises(hipdrv.Yolo2HipError, match="aspect too extreme"):
        hipdrv.letterbox_u8(yuv420ref.to_rgb(frame, fmt))
    with pytest.raises(hipdrv.Yolo2HipError, match="aspect too extreme"):
        hipdrv.letterbox_pix(frame, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_single_image_entries_take_a_frame_at_any_address(fmt):
    L = hipdrv.lib()
    w, h = 34, 18
    frame, rgb = frame_set(fmt)[4], rgb_set()[4]
    expect = want(("letterbox", 4), lambda: hipdrv.letterbox_u8(rgb))
    dets = np.zeros(1, dtype=hipdrv.DET_DTYPE)
    dets[0] = (0, 0, 3, 0.9, 0.5, 0.5, 0.6, 0.6)
    painted, n_drawn = hipdrv.annotate_pix(rgb, dets, "rgb24", thresh=0.2, labels=NAMES)
    assert n_drawn == 1
    lab, n_labels, _keep = hipdrv._label_args(NAMES)
    out = hipdrv.DevBuf(nbytes=3 * 416 * 416 * 4)
    ann = hipdrv.DevBuf(nbytes=w * h * 3)
    for shift in (1, 2, 3):
        buf = hipdrv.DevBuf(np.concatenate([np.zeros(shift, dtype=np.uint8), frame.reshape(-1)]))
        assert L.yolo2_hip_letterbox_pix(buf.addr + shift, w, h, hipdrv.pix_code(fmt), out.addr, 416, 416, None) == 0, L.yolo2_hip_last_error()
        assert _same_bits(out.get(np.float32, (3, 416, 416)), expect), shift
        assert L.yolo2_hip_annotate_pix(buf.addr + shift, w, h, hipdrv.pix_code(fmt), dets.ctypes.data_as(C.c_void_p), 1, C.c_float(0.2),
                                        lab, n_labels, ann.addr, None, None) == 0, L.yolo2_hip_last_error()
        assert np.array_equal(ann.get(np.uint8, (h, w, 3)), painted), shift
        buf.free()
    out.free()
    ann.free()


# ------------------------------------------------------------------ networks

@pytest.mark.parametrize("fmt", FORMATS)
def test_int16_region_equals_the_rgb_entry(ctx, fmt):
    frames, rgb = frame_set(fmt), rgb_set()
    for batch, pick in ((1, lambda s: s[4:6]), (BATCH, seven)):
        expect, qw = want(("i16", batch), lambda: ctx.run_images_host(pick(rgb), batch, pixfmt="rgb24"))
        got, q = ctx.run_images_host(pick(frames), batch, pixfmt=fmt)
        assert q == qw
        assert np.array_equal(got, expect), (fmt, batch)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
def test_f16_region_bitwise_equals_the_rgb_entry(ctx, fmt, split):
    frames, rgb = frame_set(fmt), rgb_set()
    tag = "<split>" if split else ""
    for batch, pick in ((1, lambda s: s[4:6]), (BATCH, seven)):
        got = ctx.run_images_f16_host(pick(frames), batch, split=bool(split), pixfmt=fmt)
        assert ctx.images_layer0_kernel(split) == f"k_conv0_pool_mfma_{fmt}{tag}"
        expect = ctx.run_images_f16_host(pick(rgb), batch, split=bool(split), pixfmt="rgb24")
        assert ctx.images_layer0_kernel(split) == "k_conv0_pool_mfma_u8" + tag      # after an RGB24 call: the byte kernel again
        assert _same_bits(got, expect), (fmt, split, batch)


@pytest.mark.parametrize("split", [0, 1])
def test_f16_no_mfma0_takes_the_formats_letterbox_route(model, split):
    c = hipdrv.Yolo2Hip(0)
    c.set_option("f16_no_mfma0", 1)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    frame_kernel = "k_conv0_pool_f16<split>" if split else "k_conv0_pool_f16"
    expect = c.run_images_f16_host(seven(rgb_set()), BATCH, split=bool(split), pixfmt="rgb24")
    assert c.images_layer0_kernel(split) == "k_letterbox_u8_batch + " + frame_kernel
    for fmt in FORMATS:
        got = c.run_images_f16_host(seven(frame_set(fmt)), BATCH, split=bool(split), pixfmt=fmt)
        assert c.images_layer0_kernel(split) == f"k_letterbox_{fmt}_batch + " + frame_kernel
        assert _same_bits(got, expect), (fmt, split)
    c.run_images_f16_host(rgb_set()[:1], 1, split=bool(split), pixfmt="rgb24")
    assert c.images_layer0_kernel(split) == "k_letterbox_u8_batch + " + frame_kernel
    c.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_int8_region_bitwise_equals_the_rgb_entry(ctx8, fmt):
    frames, rgb = frame_set(fmt), rgb_set()
    for batch, pick in ((1, lambda s: s[4:6]), (BATCH, seven)):
        got = ctx8.run_images_int8_host(pick(frames), batch, pixfmt=fmt)
        assert ctx8.images_front_kernel_int8() == "k_i8_front_" + fmt
        expect = want(("i8", batch), lambda: ctx8.run_images_int8_host(pick(rgb), batch, pixfmt="rgb24"))
        assert _same_bits(got, expect), (fmt, batch)
    ctx8.run_images_int8_host(rgb[:1], 1, pixfmt="rgb24")
    assert ctx8.images_front_kernel_int8() == "k_i8_front_u8"
    ctx8.set_option("i8_no_front", 1)
    try:
        got = ctx8.run_images_int8_host(seven(frames), BATCH, pixfmt=fmt)
        assert ctx8.images_front_kernel_int8() == f"k_letterbox_{fmt}_batch + k_i8_quant_input + k_conv_i8"
        assert _same_bits(got, want(("i8", BATCH), None))
        ctx8.run_images_int8_host(rgb[:1], 1, pixfmt="rgb24")
        assert ctx8.images_front_kernel_int8() == "k_letterbox_u8_batch + k_i8_quant_input + k_conv_i8"
    finally:
        ctx8.set_option("i8_no_front", None)


def _same_records(a, b, n):
    assert np.array_equal(a["counts"], b["counts"])
    for f in range(n):
        assert a["dets"][f].tobytes() == b["dets"][f].tobytes(), f
    assert a["final_q"] == b["final_q"]


@pytest.mark.parametrize("precision", ["int16", "fp16", "fp32fast", "int8"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_records_equal_the_rgb_entries(ctx, ctx8, fmt, precision):
    c = ctx8 if precision == "int8" else ctx
    frames, rgb = seven(frame_set(fmt)), seven(rgb_set())
    expect = want(("dets", precision), lambda: hipdrv.run_images_dets(c._h, rgb, BATCH, THRESH, NMS, cap=CAP, precision=precision, pixfmt="rgb24"))
    assert int(expect["counts"].sum()) > 10
    got = hipdrv.run_images_dets(c._h, frames, BATCH, THRESH, NMS, cap=CAP, precision=precision, pixfmt=fmt)
    _same_records(got, expect, len(frames))


# ------------------------------------------------------------------ painting and the loop

def _two_calls(ctx, precision):
    """the RGB24 route: records from the _pix_dets entry, then both annotate entries, on the conversion"""
    def make():
        rgb = seven(rgb_set())
        r = hipdrv.run_images_dets(ctx._h, rgb, BATCH, THRESH, NMS, cap=CAP, precision=precision, pixfmt="rgb24")
        painted, drawn = ctx.annotate_images(rgb, r["dets"], None, BATCH, THRESH, labels=NAMES, pixfmt="rgb24")
        jpg, drawn_j = ctx.annotate_images(rgb, r["dets"], None, BATCH, THRESH, labels=NAMES, pixfmt="rgb24", jpeg_quality=80)
        assert list(drawn) == list(drawn_j) and int(sum(drawn)) >= 10, list(drawn)      # something is painted
        return r, painted, jpg, [int(d) for d in drawn]
    return want(("two", precision), make)


@pytest.mark.parametrize("fmt", FORMATS)
def test_annotated_frames_and_jpeg_equal_the_rgb_entries(ctx, fmt):
    frames = seven(frame_set(fmt))
    r, painted, jpg, drawn = _two_calls(ctx, "int16")
    got, n = ctx.annotate_images(frames, r["dets"], None, BATCH, THRESH, labels=NAMES, pixfmt=fmt)
    assert [int(d) for d in n] == drawn
    for f in range(len(frames)):
        assert np.array_equal(got[f], painted[f]), f
    got_j, n = ctx.annotate_images(frames, r["dets"], None, BATCH, THRESH, labels=NAMES, pixfmt=fmt, jpeg_quality=80)
    assert [int(d) for d in n] == drawn and got_j == jpg
    one, n1 = hipdrv.annotate_pix(frames[0], r["dets"][0], fmt, thresh=THRESH, labels=NAMES)      # the single-image entry, 640 x 480
    assert n1 == drawn[0] and np.array_equal(one, painted[0])


@pytest.mark.parametrize("out", ["rgb24", "jpeg"])
@pytest.mark.parametrize("precision", ["int16", "fp16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_loop_equals_pix_dets_and_annotate_on_the_conversion(ctx, fmt, precision, out):
    frames = seven(frame_set(fmt))
    r, painted, jpg, drawn = _two_calls(ctx, precision)
    got = ctx.loop_images(frames, pixfmt=fmt, precision=precision, thresh=THRESH, nms=NMS, labels=NAMES, jpeg_quality=80 if out == "jpeg" else None,
                          batch=BATCH, cap=CAP)
    assert np.array_equal(got["counts"], r["counts"]) and got["final_q"] == r["final_q"]
    assert [int(d) for d in got["drawn"]] == drawn
    for f in range(len(frames)):
        assert got["dets"][f].tobytes() == r["dets"][f].tobytes(), f
        assert got["frames"][f] == jpg[f] if out == "jpeg" else np.array_equal(got["frames"][f], painted[f]), f
    info = ctx.loop_last_info()
    assert info["image_bytes_staged"] == sum(im.nbytes for im in frames)      # 1.5 bytes per pixel went up
    if precision == "fp16":
        assert ctx.images_layer0_kernel(False) == "k_conv0_pool_mfma_" + fmt


# ------------------------------------------------------------------ multi-GPU

@pytest.mark.parametrize("fmt", FORMATS)
def test_multi_context_equals_the_single_context(ctx, model, fmt):
    """one multi-context call per entry over two contexts on device 0, as tests/test_gpu_post_multi.py does"""
    frames, rgb = seven(frame_set(fmt)), seven(rgb_set())
    r, painted, jpg, drawn = _two_calls(ctx, "int16")
    m = hipdrv.Yolo2HipMulti([0, 0])
    m.load_model(model)
    region, q = m.run_images(frames, 2, pixfmt=fmt)
    expect, qw = want(("multi_i16",), lambda: m.run_images(rgb, 2, pixfmt="rgb24"))
    assert q == qw and np.array_equal(region, expect)
    got = m.loop_images(frames, batch_per_device=2, pixfmt=fmt, precision="int16", thresh=THRESH, nms=NMS, labels=NAMES, cap=CAP)
    m.close()
    assert np.array_equal(got["counts"], r["counts"]) and got["final_q"] == r["final_q"]
    for f in range(len(frames)):
        assert got["dets"][f].tobytes() == r["dets"][f].tobytes() and (got["dets"][f]["frame"] == f).all(), f
        assert np.array_equal(got["frames"][f], painted[f]), f


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_launch_nothing_and_the_next_call_is_unaffected(model, fmt):
    L = hipdrv.lib()
    code = hipdrv.pix_code(fmt)
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    good = frame_set(fmt)[4]      # 34 x 18
    n, ptrs, ws, hs, fcode, keep = hipdrv._image_args([good, good], fmt)
    assert fcode == code and list(ws) == [34, 34] and list(hs) == [18, 18]
    odd_w, odd_h = (C.c_int * 2)(34, 33), (C.c_int * 2)(18, 17)
    null_img = (C.c_void_p * 2)(ptrs[0], None)
    reg16 = np.zeros((2, 425, 13, 13), dtype=np.int16)
    regf = np.zeros((2, 425, 13, 13), dtype=np.float32)
    dets = np.zeros((2, 8), dtype=hipdrv.DET_DTYPE)
    counts = np.zeros(2, dtype=np.int32)
    outs = [np.full(34 * 18 * 3, 0xA5, dtype=np.uint8) for _ in range(2)]
    optrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    caps, sizes = np.full(2, 34 * 18 * 3, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    q = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    entries = {
        "host": lambda p, w, h, f: L.yolo2_hip_run_images_pix_host(c._h, p, w, h, f, 2, 1, vp(reg16), C.byref(q)),
        "dets": lambda p, w, h, f: L.yolo2_hip_run_images_pix_dets(c._h, p, w, h, f, 2, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts), C.byref(q)),
        "f16_host": lambda p, w, h, f: L.yolo2_hip_run_images_pix_f16_host(c._h, 0, p, w, h, f, 2, 1, vp(regf)),
        "dets_f16": lambda p, w, h, f: L.yolo2_hip_run_images_pix_dets_f16(c._h, 1, p, w, h, f, 2, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts)),
        "int8": lambda p, w, h, f: L.yolo2_hip_run_images_pix_int8_host(c._h, p, w, h, f, 2, 1, vp(regf)),
        "annotate": lambda p, w, h, f: L.yolo2_hip_annotate_images_pix_host(c._h, p, w, h, f, 2, 1, vp(dets), 8, vp(counts), C.c_float(0.2), None, 0, optrs, None),
        "loop": lambda p, w, h, f: L.yolo2_hip_loop_images_pix(c._h, 0, p, w, h, f, 2, 1, C.c_float(0.05), C.c_float(0.45), hipdrv.DETS_BEST_CLASS, vp(dets), 8,
                                                               vp(counts), None, None, 0, 0, 80, optrs, vp(caps), vp(sizes), None),
    }
    for name, call in entries.items():
        cases = [((ptrs, odd_w, hs, code), b"even width, not 33"), ((ptrs, ws, odd_h, code), b"even height, not 17"),
                 ((ptrs, ws, hs, code ^ 0x100), b"unknown pixel format"), ((null_img, ws, hs, code), b"null")]
        if name == "int8":      # no int8 weights on this context: that is refused first, except for what is checked before it
            cases = cases[2:3]
        for args, text in cases:
            assert call(*args) == hipdrv.YOLO2_ERROR, (name, text)
            assert text in L.yolo2_hip_last_error(), (name, text, L.yolo2_hip_last_error())
    assert c.images_layer0_kernel(0) == "" and c.images_layer0_kernel(1) == "" and c.images_front_kernel_int8() == ""      # no pass ran
    assert not reg16.any() and not regf.any() and not counts.any() and not sizes.any() and all((o == 0xA5).all() for o in outs)
    # the standalone letterbox: odd sizes, null
    out = hipdrv.DevBuf(nbytes=3 * 416 * 416 * 4)
    buf = hipdrv.DevBuf(good)
    for (w, h), text in (((33, 18), b"even width, not 33"), ((34, 17), b"even height, not 17")):
        assert L.yolo2_hip_letterbox_pix(buf.addr, w, h, code, out.addr, 416, 416, None) == hipdrv.YOLO2_ERROR
        assert text in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(0, 34, 18, code, out.addr, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert not out.get(np.float32, (3, 416, 416)).any()
    buf.free()
    out.free()
    # the context still works after the refusals
    got, _ = c.run_images_host([good], 1, pixfmt=fmt)
    expect, _ = c.run_images_host([rgb_set()[4]], 1, pixfmt="rgb24")
    assert np.array_equal(got, expect)
    c.close()


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_nv12_and_yuv420p_streams_give_the_rgb_streams_records(model, tmp_path):
    """5 raw frames of 64 x 48 as NV12 and as yuv420p against the RGB24 file of the converted frames: the same JSONL"""
    w, h = 64, 48
    ys, xs = np.arange(h) * DOG.shape[0] // h, np.arange(w) * DOG.shape[1] // w
    base = DOG[ys][:, xs]
    pictures = [np.ascontiguousarray(np.roll(base, 6 * k, axis=1)) for k in range(5)]
    nv12 = [yuv420ref.from_rgb(p, "nv12") for p in pictures]
    i420 = [yuv420ref.from_rgb(p, "i420") for p in pictures]
    (tmp_path / "video.nv12").write_bytes(b"".join(f.tobytes() for f in nv12) + b"\x00" * 100)      # a trailing partial frame is dropped
    (tmp_path / "video.i420").write_bytes(b"".join(f.tobytes() for f in i420))
    (tmp_path / "video.rgb").write_bytes(b"".join(yuv420ref.to_rgb(f, "nv12").tobytes() for f in nv12))
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    size = ["--video-width", str(w), "--video-height", str(h)]
    dets = 0
    # int16: all three files, the yuv420p run also through the writer's host route (no --annotate-gpu: the host restatement converts the
    # frame); fp16 on two contexts: "i420" as the other spelling
    runs = (("i16", ["--precision", "int16"], (("rgb", "rgb24", []), ("nv12", "nv12", []), ("i420", "yuv420p", ["--save-annotated-dir", str(tmp_path / "ann")]))),
            ("f16_multi", ["--precision", "fp16", "--devices", "0,0"], (("rgb", "rgb24", []), ("i420", "i420", []))))
    for tag, extra, files in runs:
        common = ["--weights", str(tmp_path / "weights"), "--batch", "2", "--thresh", "0.05", "--chunk-batches", "1"] + extra + size
        out = {}
        for ext, spelled, more in files:
            path = tmp_path / f"{tag}_{ext}.jsonl"
            r = _cli(common + more + ["--video-raw", str(tmp_path / f"video.{ext}"), "--video-pix-fmt", spelled, "--jsonl", str(path)], tmp_path)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "Streaming inference completed successfully (5 inference frames" in r.stdout
            out[ext] = [json.loads(line) for line in path.read_text().splitlines()]
        for ext in out:
            if ext == "rgb":
                continue
            assert len(out[ext]) == 5
            for a, b in zip(out[ext], out["rgb"]):
                a, b = dict(a), dict(b)
                assert a.pop("source").endswith("video." + ext) and b.pop("source").endswith("video.rgb")
                assert a == b, (tag, ext)
                dets += len(a["detections"])
    print("detections compared:", dets)
    assert dets > 0
    assert len((tmp_path / "ann" / "frame_000001.ppm").read_bytes()) > w * h * 3


def test_calibrate_tool_takes_the_same_streams(model, tmp_path):
    """yolov2_calibrate --video-raw: the int16 weight set from 4 NV12 / yuv420p frames is the one from their RGB24 conversion, byte for byte"""
    w, h = 64, 48
    ys, xs = np.arange(h) * DOG.shape[0] // h, np.arange(w) * DOG.shape[1] // w
    pictures = [np.ascontiguousarray(np.roll(DOG[ys][:, xs], 9 * k, axis=1)) for k in range(4)]
    nv12 = [yuv420ref.from_rgb(p, "nv12") for p in pictures]
    (tmp_path / "video.nv12").write_bytes(b"".join(f.tobytes() for f in nv12))
    (tmp_path / "video.i420").write_bytes(b"".join(yuv420ref.from_rgb(p, "i420").tobytes() for p in pictures))
    (tmp_path / "video.rgb").write_bytes(b"".join(yuv420ref.to_rgb(f, "nv12").tobytes() for f in nv12))
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=False)
    blobs = {}
    for ext, spelled in (("rgb", "rgb24"), ("nv12", "nv12"), ("i420", "yuv420p")):
        r = subprocess.run([os.path.join(PKG, "yolov2_calibrate"), "--weights", str(tmp_path / "weights"), "--video-raw", str(tmp_path / f"video.{ext}"),
                            "--video-width", str(w), "--video-height", str(h), "--video-pix-fmt", spelled, "--batch", "3", "--out", str(tmp_path / ext)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "calibrated on 4 images" in r.stdout
        blobs[ext] = {name: (tmp_path / ext / name).read_bytes() for name in hipdrv.CalibratedModel.FILES}
    assert blobs["nv12"] == blobs["rgb"] and blobs["i420"] == blobs["rgb"]
