"""GPU tests of the packed RGB formats: BGR24, RGBA32 and BGRA32 frames through every _pix entry (letterbox, int16 / fp16 / split-fp16 /
int8 region tensors, detection records, the painter, annotated JPEG, the loop, a multi context, calibration, the CLI) are bit-identical
to the RGB24 entries fed the same pixels with the bytes reordered, and the loop's YOLO2_LOOP_OUT_BGR24 frames are its RGB24 frames with
bytes 0 and 2 of every pixel exchanged.  The expected side is always an RGB24 entry of the same build on packedref.to_rgb(frame) - those
entries are pinned to the reference by the tests of their own - never the code under test.  One test (constant frames) does not go
through packedref at all, so that a kernel and a helper that share a wrong permutation are caught."""
import json
import os
import subprocess

import numpy as np
import pytest

import jpegdec_cases as jc
import orclib
import packedref
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
NAMES = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
FORMATS = packedref.FORMATS
WIDE = ("rgba32", "bgra32")
C = hipdrv.C
THRESH, NMS, BATCH, CAP = 0.07, 0.45, 3, 845
TOO_NARROW = ((2, 1000), (1000, 2))
# (w, h) of the random frames: 3 x 5 has BGR24 rows of 9 bytes, which start on every alignment mod 4; 3 x 1000 and 1000 x 3 fit the
# canvas with 1 pixel (the c == new_w - 1 branch)
RANDOM = ((1, 1), (2, 2), (5, 3), (3, 5), (3, 1000), (1000, 3), (33, 17))
NATURAL = ((641, 479), (300, 700))


def _natural_rgb(w, h):
    """the dog picture resampled to w x h (nearest)"""
    ys, xs = np.arange(h) * DOG.shape[0] // h, np.arange(w) * DOG.shape[1] // w
    return np.ascontiguousarray(DOG[ys][:, xs])


def _random(w, h, fmt):
    return packedref.random_frame(np.random.default_rng(w * 10007 + h), w, h, fmt)


_sets = {}


def frame_set(fmt):
    """the issue's frames that can be letterboxed, the same pictures in every format, the fourth byte random"""
    if fmt not in _sets:
        rng = np.random.default_rng(99)
        _sets[fmt] = [_random(w, h, fmt) for w, h in RANDOM] + \
                     [packedref.from_rgb(_natural_rgb(w, h), fmt, rng.integers(0, 256, (h, w), dtype=np.uint8)) for w, h in NATURAL]
    return _sets[fmt]


def seven(frames):
    """batch 3 over 7 frames: a ragged last chunk, mixed sizes in every chunk"""
    return [frames[k] for k in (7, 0, 4, 8, 2, 5, 6)]


_rgb = []


def rgb_set():
    """the reorder of the set: the expected side's input.  Computed once, from the BGR24 frames; the other formats hold the same pictures."""
    if not _rgb:
        _rgb.extend(packedref.to_rgb(f, "bgr24") for f in frame_set("bgr24"))
        for fmt in WIDE:
            for a, f in zip(_rgb, frame_set(fmt)):
                assert np.array_equal(a, packedref.to_rgb(f, fmt))
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
    """an RGB24 entry's result, computed once and shared by the formats' tests"""
    if key not in _want:
        _want[key] = make()
    return _want[key]


# ------------------------------------------------------------------ letterbox

@pytest.mark.parametrize("fmt", FORMATS)
def test_channel_order_of_a_constant_frame(fmt):
    """R = 10, G = 20, B = 30 written by hand in each format's byte order (no helper): planes 0, 1, 2 are 10 / 255, 20 / 255, 30 / 255.
    A 1 x 1 frame takes no interpolation: exact bits.  An 8 x 6 frame interpolates between equal values, (1 - d) v + d v in fp32: three
    roundings of a value below 0.125 (ulp 7.5e-9) per pass, two passes - within 5e-8, while the channels are 0.039 apart."""
    pixel = {"bgr24": [30, 20, 10], "rgba32": [10, 20, 30, 77], "bgra32": [30, 20, 10, 77]}[fmt]
    expect = [np.float32(v) / np.float32(255) for v in (10, 20, 30)]
    one = hipdrv.letterbox_pix(np.array(pixel, dtype=np.uint8).reshape(1, 1, -1), fmt)
    for k in range(3):
        assert (one[k].view(np.uint32) == expect[k].view(np.uint32)).all(), (fmt, k)
    frame = np.ascontiguousarray(np.broadcast_to(np.array(pixel, dtype=np.uint8), (6, 8, len(pixel))))
    lb = hipdrv.letterbox_pix(frame, fmt)
    rows = slice((416 - 312) // 2, (416 - 312) // 2 + 312)      # the fitted area of an 8 x 6 picture: 416 x 312
    for k in range(3):
        assert np.abs(lb[k, rows] - expect[k]).max() <= 5e-8, (fmt, k)
        assert (lb[k, :rows.start] == 0.5).all() and (lb[k, rows.stop:] == 0.5).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_letterbox_pix_bit_identical_to_letterbox_u8_of_the_reorder(fmt):
    for k, (frame, rgb) in enumerate(zip(frame_set(fmt), rgb_set())):
        expect = want(("letterbox", k), lambda: hipdrv.letterbox_u8(rgb))
        assert _same_bits(hipdrv.letterbox_pix(frame, fmt), expect), (fmt, frame.shape)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", TOO_NARROW)
def test_frames_that_fit_with_no_pixel_are_refused_like_their_reorder(fmt, w, h):
    frame = _random(w, h, fmt)
    with pytest.raises(hipdrv.Yolo2HipError, match="aspect too extreme"):
        hipdrv.letterbox_u8(packedref.to_rgb(frame, fmt))
    with pytest.raises(hipdrv.Yolo2HipError, match="aspect too extreme"):
        hipdrv.letterbox_pix(frame, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_single_image_entries_and_the_address_of_a_frame(fmt):
    """BGR24 works at address shifts 1, 2 and 3; a 32-bit frame off its 4-byte boundary is refused and nothing is launched"""
    L = hipdrv.lib()
    w, h = 33, 17
    frame, rgb = frame_set(fmt)[6], rgb_set()[6]
    expect = want(("letterbox", 6), lambda: hipdrv.letterbox_u8(rgb))
    dets = np.zeros(1, dtype=hipdrv.DET_DTYPE)
    dets[0] = (0, 0, 3, 0.9, 0.5, 0.5, 0.6, 0.6)
    painted, n_drawn = hipdrv.annotate_pix(rgb, dets, "rgb24", thresh=0.2, labels=NAMES)
    assert n_drawn == 1
    lab, n_labels, _keep = hipdrv._label_args(NAMES)
    out = hipdrv.DevBuf(np.zeros(3 * 416 * 416, dtype=np.float32))
    ann = hipdrv.DevBuf(np.zeros(w * h * 3, dtype=np.uint8))
    for shift in (1, 2, 3):
        buf = hipdrv.DevBuf(np.concatenate([np.zeros(shift, dtype=np.uint8), frame.reshape(-1)]))
        rc_l = L.yolo2_hip_letterbox_pix(buf.addr + shift, w, h, hipdrv.pix_code(fmt), out.addr, 416, 416, None)
        err_l = L.yolo2_hip_last_error()
        rc_a = L.yolo2_hip_annotate_pix(buf.addr + shift, w, h, hipdrv.pix_code(fmt), dets.ctypes.data_as(C.c_void_p), 1, C.c_float(0.2),
                                        lab, n_labels, ann.addr, None, None)
        err_a = L.yolo2_hip_last_error()
        if fmt == "bgr24":
            assert rc_l == 0 and rc_a == 0, (err_l, err_a)
            assert _same_bits(out.get(np.float32, (3, 416, 416)), expect), shift
            assert np.array_equal(ann.get(np.uint8, (h, w, 3)), painted), shift
        else:
            assert rc_l == hipdrv.YOLO2_ERROR and b"frame starts on a 4-byte boundary" in err_l and fmt.upper().encode() in err_l
            assert rc_a == hipdrv.YOLO2_ERROR and b"frame starts on a 4-byte boundary" in err_a
            assert not out.get(np.float32, (3, 416, 416)).any() and not ann.get(np.uint8, (h, w, 3)).any()      # nothing ran
        buf.free()
    out.free()
    ann.free()


# ------------------------------------------------------------------ the fourth byte

@pytest.mark.parametrize("fmt", WIDE)
def test_the_fourth_byte_reaches_no_result(ctx, fmt):
    """frames that differ only in X (0x00, 0xff, random): the same letterbox bits, fp16 region bits and painted frames"""
    rgb = [rgb_set()[k] for k in (6, 7, 3)]      # 33 x 17, 641 x 479, 3 x 5
    rng = np.random.default_rng(4)
    variants = [[packedref.from_rgb(p, fmt, x(p)) for p in rgb]
                for x in (lambda p: 0x00, lambda p: 0xff, lambda p: rng.integers(0, 256, p.shape[:2], dtype=np.uint8))]
    assert not np.array_equal(variants[0][0], variants[1][0])
    dets = np.zeros((3, 2), dtype=hipdrv.DET_DTYPE)
    for f in range(3):
        dets[f, 0] = (f, 0, 3, 0.9, 0.5, 0.5, 0.6, 0.6)
        dets[f, 1] = (f, 0, 5, 0.8, 0.3, 0.3, 0.2, 0.3)
    results = []
    for frames in variants:
        lb = [hipdrv.letterbox_pix(f, fmt) for f in frames]
        region = ctx.run_images_f16_host(frames, 2, pixfmt=fmt)
        painted, drawn = ctx.annotate_images(frames, dets, [2, 2, 2], 2, 0.2, labels=NAMES, pixfmt=fmt)
        assert [int(d) for d in drawn] == [2, 2, 2]
        results.append((lb, region, painted))
    for lb, region, painted in results[1:]:
        assert all(_same_bits(a, b) for a, b in zip(lb, results[0][0]))
        assert _same_bits(region, results[0][1])
        assert all(np.array_equal(a, b) for a, b in zip(painted, results[0][2]))
    expect, _ = ctx.annotate_images(rgb, dets, [2, 2, 2], 2, 0.2, labels=NAMES, pixfmt="rgb24")
    assert all(np.array_equal(a, b) for a, b in zip(results[0][2], expect))


# ------------------------------------------------------------------ networks

@pytest.mark.parametrize("fmt", FORMATS)
def test_int16_region_equals_the_rgb_entry(ctx, fmt):
    frames, rgb = frame_set(fmt), rgb_set()
    for batch, pick in ((1, lambda s: s[6:8]), (BATCH, seven)):
        expect, qw = want(("i16", batch), lambda: ctx.run_images_host(pick(rgb), batch, pixfmt="rgb24"))
        got, q = ctx.run_images_host(pick(frames), batch, pixfmt=fmt)
        assert q == qw
        assert np.array_equal(got, expect), (fmt, batch)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
def test_f16_region_bitwise_equals_the_rgb_entry(ctx, fmt, split):
    frames, rgb = frame_set(fmt), rgb_set()
    tag = "<split>" if split else ""
    for batch, pick in ((1, lambda s: s[6:8]), (BATCH, seven)):
        got = ctx.run_images_f16_host(pick(frames), batch, split=bool(split), pixfmt=fmt)
        assert ctx.images_layer0_kernel(split) == f"k_conv0_pool_mfma_{fmt}{tag}"      # the format's own kernel ran
        expect = want(("f16", split, batch), lambda: ctx.run_images_f16_host(pick(rgb), batch, split=bool(split), pixfmt="rgb24"))
        assert _same_bits(got, expect), (fmt, split, batch)
    ctx.run_images_f16_host(rgb[:1], 1, split=bool(split), pixfmt="rgb24")
    assert ctx.images_layer0_kernel(split) == "k_conv0_pool_mfma_u8" + tag      # after an RGB24 call: the byte kernel again


@pytest.mark.parametrize("split", [0, 1])
def test_f16_no_mfma0_takes_the_formats_letterbox_route(ctx, model, split):
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
    c.close()
    # ... and agrees with the fused kernels.  Not bit for bit: under f16_no_mfma0 layer 0 is the fp32 VALU kernel, fused it is the MFMA
    # kernel, and the two sum in different orders on RGB24 input already (tests/test_gpu_parity.py,
    # test_f32tol_layer0_on_mfma_agrees_with_its_fp32_valu_form).  The bound is the triangle inequality over the project's bounds of each
    # pass against fp32: 0.03 per fp16 pass (test_fp16_mfma_path_vs_fp32_reference) -> 0.06, 1e-3 per split pass -> 2e-3.
    fused = want(("f16", split, BATCH), lambda: ctx.run_images_f16_host(seven(rgb_set()), BATCH, split=bool(split), pixfmt="rgb24"))
    # (frame 5 of the seven, 1000 x 3, is fitted 1 pixel high: the letterbox's row scale divides by zero there, as for RGB24, and its
    #  tensor is NaN on every route - the same elements on both)
    assert np.array_equal(np.isnan(expect), np.isnan(fused)) and not np.isnan(expect[[0, 1, 2, 3, 4, 6]]).any()
    diff = float(np.nanmax(np.abs(expect - fused)))
    print("f16_no_mfma0 against fused, split", split, "max |diff|", diff)
    assert diff <= (2e-3 if split else 0.06)
    assert not np.array_equal(expect, fused), "the option did not change layer 0's kernel"


@pytest.mark.parametrize("fmt", FORMATS)
def test_int8_region_bitwise_equals_the_rgb_entry(ctx8, fmt):
    frames, rgb = frame_set(fmt), rgb_set()
    for batch, pick in ((1, lambda s: s[6:8]), (BATCH, seven)):
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
        assert _same_bits(got, want(("i8", BATCH), None))      # agrees with the fused kernel
    finally:
        ctx8.set_option("i8_no_front", None)


def _same_records(a, b, n):
    assert np.array_equal(a["counts"], b["counts"])
    for f in range(n):
        assert a["dets"][f].tobytes() == b["dets"][f].tobytes(), f
    assert a["final_q"] == b["final_q"]


@pytest.mark.parametrize("tail", ["core", "app"])
@pytest.mark.parametrize("precision", ["int16", "fp16", "fp32fast", "int8"])
def test_records_equal_the_rgb_entries(ctx, ctx8, precision, tail):
    c = ctx8 if precision == "int8" else ctx
    rgb = seven(rgb_set())
    expect = hipdrv.run_images_dets(c._h, rgb, BATCH, THRESH, NMS, cap=CAP, precision=precision, pixfmt="rgb24", tail=tail)
    assert int(expect["counts"].sum()) > 10
    for fmt in FORMATS:
        got = hipdrv.run_images_dets(c._h, seven(frame_set(fmt)), BATCH, THRESH, NMS, cap=CAP, precision=precision, pixfmt=fmt, tail=tail)
        _same_records(got, expect, len(rgb))


# ------------------------------------------------------------------ painting and the loop

def _two_calls(ctx, precision):
    """the RGB24 route: records from the _pix_dets entry, then both annotate entries, on the reorder"""
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
    for f in (0, 2, 6):      # the single-image entry: 641 x 479, 3 x 1000 (runs that cross rows), 33 x 17
        one, n1 = hipdrv.annotate_pix(frames[f], r["dets"][f], fmt, thresh=THRESH, labels=NAMES)
        assert n1 == drawn[f] and np.array_equal(one, painted[f]), f


@pytest.mark.parametrize("out", ["rgb24", "jpeg"])
@pytest.mark.parametrize("precision", ["int16", "fp16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_loop_equals_pix_dets_and_annotate_on_the_reorder(ctx, fmt, precision, out):
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
    assert info["image_bytes_staged"] == sum(im.nbytes for im in frames)      # 3 / 4 bytes per pixel went up
    if precision == "fp16":
        assert ctx.images_layer0_kernel(False) == "k_conv0_pool_mfma_" + fmt


@pytest.mark.parametrize("precision", ["int16", "fp16"])
@pytest.mark.parametrize("fmt", ["rgb24", "bgr24", "bgra32"])
def test_loop_bgr24_output_is_the_rgb24_output_with_the_bytes_exchanged(ctx, fmt, precision):
    frames = seven(rgb_set() if fmt == "rgb24" else frame_set(fmt))
    r, painted, jpg, drawn = _two_calls(ctx, precision)
    got = ctx.loop_images(frames, pixfmt=fmt, precision=precision, thresh=THRESH, nms=NMS, labels=NAMES, batch=BATCH, cap=CAP, out_order="bgr")
    assert np.array_equal(got["counts"], r["counts"]) and [int(d) for d in got["drawn"]] == drawn
    for f in range(len(frames)):
        assert got["dets"][f].tobytes() == r["dets"][f].tobytes(), f
        assert np.array_equal(got["frames"][f], painted[f][..., ::-1]), f


def test_loop_bgr24_output_from_jpeg_streams_and_format_2_stays_refused(ctx):
    names = ["jpg/base_420", "jpg/grey", "jpg/base_422", "jpg/restart_rows"]
    streams = [jc.stream(n) for n in names]
    kw = dict(precision="int16", tail="app", thresh=0.005, nms=NMS, labels=NAMES, batch=BATCH)
    expect = ctx.loop_jpegs(streams, **kw)
    assert expect["drawn"].max() > 0
    got = ctx.loop_jpegs(streams, out_order="bgr", **kw)
    assert not got["status"].any() and np.array_equal(got["counts"], expect["counts"]) and np.array_equal(got["drawn"], expect["drawn"])
    for f in range(len(streams)):
        assert got["dets"][f].tobytes() == expect["dets"][f].tobytes(), f
        assert np.array_equal(got["frames"][f], expect["frames"][f][..., ::-1]), f
    # the value 2 is no format, for frames and for streams
    L = hipdrv.lib()
    frames = rgb_set()[6:8]
    caps = [im.shape[0] * im.shape[1] * 3 for im in frames]
    rc, dets, counts, q, outs, sizes, dr = hipdrv.loop_images_raw(ctx._h, frames, "rgb24", 0, hipdrv.DETS_BEST_CLASS, THRESH, NMS, 2, CAP, NAMES, 2, 80,
                                                                  caps, guard=8)
    assert rc == hipdrv.YOLO2_ERROR and b"output format 2" in L.yolo2_hip_last_error()
    assert all((o == 0xA5).all() for o in outs) and not counts.any() and not sizes.any()
    full = 4 << 20
    rc = hipdrv.loop_jpegs_raw(ctx._h, streams[:2], 0, hipdrv.DETS_BEST_CLASS, THRESH, NMS, 2, CAP, NAMES, 2, 80, [full, full], guard=8)[0]
    assert rc == hipdrv.YOLO2_ERROR and b"output format 2" in L.yolo2_hip_last_error()
    # ... and a BGR24 frame needs the room an RGB24 one does
    caps[1] -= 1
    rc, dets, counts, q, outs, sizes, dr = hipdrv.loop_images_raw(ctx._h, frames, "rgb24", 0, hipdrv.DETS_BEST_CLASS, THRESH, NMS, 2, CAP, NAMES,
                                                                  hipdrv.LOOP_OUT_BGR24, 0, caps, guard=8)
    assert rc == hipdrv.YOLO2_ERROR and b"too small for frame 1" in L.yolo2_hip_last_error()
    assert all((o == 0xA5).all() for o in outs)


# ------------------------------------------------------------------ multi-GPU and calibration

@pytest.mark.parametrize("fmt", FORMATS)
def test_multi_context_equals_the_single_context(ctx, model, fmt):
    """one multi-context call per entry over two contexts on device 0, as tests/test_gpu_yuv420.py does"""
    frames, rgb = seven(frame_set(fmt)), seven(rgb_set())
    r, painted, jpg, drawn = _two_calls(ctx, "int16")
    m = hipdrv.Yolo2HipMulti([0, 0])
    m.load_model(model)
    region, q = m.run_images(frames, 2, pixfmt=fmt)
    expect, qw = want(("multi_i16",), lambda: m.run_images(rgb, 2, pixfmt="rgb24"))
    assert q == qw and np.array_equal(region, expect)
    got = m.loop_images(frames, batch_per_device=2, pixfmt=fmt, precision="int16", thresh=THRESH, nms=NMS, labels=NAMES, cap=CAP)
    bgr = m.loop_images(frames, batch_per_device=2, pixfmt=fmt, precision="int16", thresh=THRESH, nms=NMS, labels=NAMES, cap=CAP, out_order="bgr")
    m.close()
    assert np.array_equal(got["counts"], r["counts"]) and got["final_q"] == r["final_q"]
    for f in range(len(frames)):
        assert got["dets"][f].tobytes() == r["dets"][f].tobytes() and (got["dets"][f]["frame"] == f).all(), f
        assert np.array_equal(got["frames"][f], painted[f]), f
        assert np.array_equal(bgr["frames"][f], painted[f][..., ::-1]), f


def test_calibration_statistics_equal_those_from_rgb24(ctx):
    """the whole set but 1000 x 3: fitted 1 pixel high, its letterboxed frame is not finite (the row scale divides by zero, for RGB24
    too), and calibration refuses such frames - from every format alike, which is checked as well"""
    pick = lambda s: [s[k] for k in (7, 0, 4, 8, 2, 1, 6, 3)]      # batch 3 over 8 frames: a ragged last chunk

    def stats(frames, fmt):
        ctx.calib_reset()
        ctx.calib_images(frames, BATCH, pixfmt=fmt)
        return ctx.calib_stats()
    expect = stats(pick(rgb_set()), "rgb24")
    assert expect["frames_seen"] == 8
    for fmt in FORMATS:
        got = stats(pick(frame_set(fmt)), fmt)
        assert got["frames_seen"] == 8
        for key in ("act_absmax", "weight_absmax", "bias_absmax"):
            assert _same_bits(got[key], expect[key]), (fmt, key)
    for fmt in ("rgb24",) + FORMATS:
        ctx.calib_reset()
        with pytest.raises(hipdrv.Yolo2HipError, match="1248 non-finite values"):      # 3 planes x 416 columns of the one fitted row
            ctx.calib_images(seven(rgb_set() if fmt == "rgb24" else frame_set(fmt)), BATCH, pixfmt=fmt)
    ctx.calib_reset()


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_launch_nothing_and_the_next_call_is_unaffected(model, fmt):
    L = hipdrv.lib()
    code = hipdrv.pix_code(fmt)
    base = hipdrv.live_bytes()
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    held = hipdrv.live_bytes()
    good = frame_set(fmt)[6]      # 33 x 17
    n, ptrs, ws, hs, fcode, keep = hipdrv._image_args([good, good], fmt)
    assert fcode == code and list(ws) == [33, 33] and list(hs) == [17, 17]
    zero_w, zero_h = (C.c_int * 2)(33, 0), (C.c_int * 2)(0, 17)
    null_img = (C.c_void_p * 2)(ptrs[0], None)
    reg16 = np.zeros((2, 425, 13, 13), dtype=np.int16)
    regf = np.zeros((2, 425, 13, 13), dtype=np.float32)
    dets = np.zeros((2, 8), dtype=hipdrv.DET_DTYPE)
    counts = np.zeros(2, dtype=np.int32)
    outs = [np.full(33 * 17 * 3, 0xA5, dtype=np.uint8) for _ in range(2)]
    optrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    caps, sizes = np.full(2, 33 * 17 * 3, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    q = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    entries = {
        "host": lambda p, w, h, f: L.yolo2_hip_run_images_pix_host(c._h, p, w, h, f, 2, 1, vp(reg16), C.byref(q)),
        "dets": lambda p, w, h, f: L.yolo2_hip_run_images_pix_dets(c._h, p, w, h, f, 2, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts), C.byref(q)),
        "f16_host": lambda p, w, h, f: L.yolo2_hip_run_images_pix_f16_host(c._h, 0, p, w, h, f, 2, 1, vp(regf)),
        "dets_f16": lambda p, w, h, f: L.yolo2_hip_run_images_pix_dets_f16(c._h, 1, p, w, h, f, 2, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts)),
        "int8": lambda p, w, h, f: L.yolo2_hip_run_images_pix_int8_host(c._h, p, w, h, f, 2, 1, vp(regf)),
        "calib": lambda p, w, h, f: L.yolo2_hip_calib_images_pix_host(c._h, p, w, h, f, 2, 1),
        "annotate": lambda p, w, h, f: L.yolo2_hip_annotate_images_pix_host(c._h, p, w, h, f, 2, 1, vp(dets), 8, vp(counts), C.c_float(0.2), None, 0, optrs, None),
        "loop": lambda p, w, h, f: L.yolo2_hip_loop_images_pix(c._h, 0, p, w, h, f, 2, 1, C.c_float(0.05), C.c_float(0.45), hipdrv.DETS_BEST_CLASS, vp(dets), 8,
                                                               vp(counts), None, None, 0, hipdrv.LOOP_OUT_BGR24, 80, optrs, vp(caps), vp(sizes), None),
    }
    twin_made = False
    for name, call in entries.items():
        cases = [((ptrs, ws, hs, code ^ 0x100), b"unknown pixel format"), ((ptrs, zero_w, hs, code), b"0x17"), ((ptrs, ws, zero_h, code), b"33x0"),
                 ((null_img, ws, hs, code), b"null")]
        if name == "int8":      # no int8 weights on this context: that is refused first, except for what is checked before it
            cases = cases[:1]
        for args, text in cases:
            assert call(*args) == hipdrv.YOLO2_ERROR, (name, text)
            assert text in L.yolo2_hip_last_error(), (name, text, L.yolo2_hip_last_error())
            # nothing is allocated for a refused call - but the split entry makes the context's split twin (its own weights, kept until
            # close) before it looks at the frames, as it does for every format: once
            if name == "dets_f16" and not twin_made and hipdrv.live_bytes() != held:
                twin_made, held = True, hipdrv.live_bytes()
            assert hipdrv.live_bytes() == held, (name, text)
    assert c.images_layer0_kernel(0) == "" and c.images_layer0_kernel(1) == "" and c.images_front_kernel_int8() == ""      # no pass ran
    assert not reg16.any() and not regf.any() and not counts.any() and not sizes.any() and all((o == 0xA5).all() for o in outs)
    # the standalone letterbox: zero size, null
    out = hipdrv.DevBuf(np.zeros(3 * 416 * 416, dtype=np.float32))
    buf = hipdrv.DevBuf(good)
    for w, h in ((0, 17), (33, 0)):
        assert L.yolo2_hip_letterbox_pix(buf.addr, w, h, code, out.addr, 416, 416, None) == hipdrv.YOLO2_ERROR
        assert b"bad image geometry" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(0, 33, 17, code, out.addr, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert not out.get(np.float32, (3, 416, 416)).any()
    buf.free()
    out.free()
    # the context still works after the refusals
    got, _ = c.run_images_host([good], 1, pixfmt=fmt)
    expect, _ = c.run_images_host([rgb_set()[6]], 1, pixfmt="rgb24")
    assert np.array_equal(got, expect)
    c.close()
    assert hipdrv.live_bytes() == base      # memory balances over the context's life


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def _pictures(n, w, h, step):
    base = _natural_rgb(w, h)
    return [np.ascontiguousarray(np.roll(base, step * k, axis=1)) for k in range(n)]


def test_cli_packed_streams_give_the_rgb_streams_records(model, tmp_path):
    """7 raw frames of 65 x 47 (odd both ways) in each format against the RGB24 file of the same pictures: the same JSONL, for int16, for
    fp16 on two contexts, and through --loop-gpu --annotate-gpu, where the annotated files are the same too"""
    w, h = 65, 47
    pictures = _pictures(7, w, h, 6)
    rng = np.random.default_rng(8)
    spell = {"rgb": "rgb24", "bgr24": "bgr24", "rgba32": "rgba", "bgra32": "bgra"}
    (tmp_path / "video.rgb").write_bytes(b"".join(p.tobytes() for p in pictures))
    for fmt in FORMATS:
        data = b"".join(packedref.from_rgb(p, fmt, rng.integers(0, 256, (h, w), dtype=np.uint8)).tobytes() for p in pictures)
        (tmp_path / f"video.{fmt}").write_bytes(data + b"\x00" * 100)      # a trailing partial frame is dropped
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    size = ["--video-width", str(w), "--video-height", str(h)]
    dets = 0
    runs = (("i16", ["--precision", "int16"], False, {}),
            ("f16_multi", ["--precision", "fp16", "--devices", "0,0"], False, {"rgba32": "rgb0", "bgra32": "bgr0"}),      # the other spellings
            ("loop", ["--precision", "fp16", "--post", "gpu", "--loop-gpu", "--annotate-gpu", "--annotated-format", "ppm"], True, {}))
    for tag, extra, annotated, respell in runs:
        common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.05", "--chunk-batches", "1"] + extra + size
        out, files = {}, {}
        for ext in ("rgb",) + FORMATS:
            path, d = tmp_path / f"{tag}_{ext}.jsonl", tmp_path / f"{tag}_{ext}"
            more = ["--save-annotated-dir", str(d)] if annotated else []
            r = _cli(common + more + ["--video-raw", str(tmp_path / f"video.{ext}"), "--video-pix-fmt", respell.get(ext, spell[ext]), "--jsonl", str(path)],
                     tmp_path)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "Streaming inference completed successfully (7 inference frames" in r.stdout
            out[ext] = [json.loads(line) for line in path.read_text().splitlines()]
            if annotated:
                files[ext] = [(n, (d / n).read_bytes()) for n in sorted(os.listdir(d))]
        for ext in FORMATS:
            assert len(out[ext]) == 7
            for a, b in zip(out[ext], out["rgb"]):
                a, b = dict(a), dict(b)
                assert a.pop("source").endswith("video." + ext) and b.pop("source").endswith("video.rgb")
                assert a == b, (tag, ext)
                dets += len(a["detections"])
            if annotated:
                assert len(files[ext]) == 7 and files[ext] == files["rgb"], (tag, ext)
    print("detections compared:", dets)
    assert dets > 0


def test_calibrate_tool_takes_the_same_streams(model, tmp_path):
    """yolov2_calibrate --video-raw: the int16 weight set from 4 frames in each format is the one from the RGB24 file, byte for byte"""
    w, h = 65, 47
    pictures = _pictures(4, w, h, 9)
    spell = {"rgb": "rgb24", "bgr24": "bgr24", "rgba32": "rgba", "bgra32": "bgr0"}
    (tmp_path / "video.rgb").write_bytes(b"".join(p.tobytes() for p in pictures))
    for fmt in FORMATS:
        (tmp_path / f"video.{fmt}").write_bytes(b"".join(packedref.from_rgb(p, fmt, 0x5a).tobytes() for p in pictures))
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=False)
    blobs = {}
    for ext in ("rgb",) + FORMATS:
        r = subprocess.run([os.path.join(PKG, "yolov2_calibrate"), "--weights", str(tmp_path / "weights"), "--video-raw", str(tmp_path / f"video.{ext}"),
                            "--video-width", str(w), "--video-height", str(h), "--video-pix-fmt", spell[ext], "--batch", "3", "--out", str(tmp_path / ext)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "calibrated on 4 images" in r.stdout
        blobs[ext] = {name: (tmp_path / ext / name).read_bytes() for name in hipdrv.CalibratedModel.FILES}
    for fmt in FORMATS:
        assert blobs[fmt] == blobs["rgb"], fmt
