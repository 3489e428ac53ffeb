"""GPU tests of the YUYV camera format: packed YUYV 4:2:2 frames through the _pix entries (letterbox, int16 / fp16 / split-fp16 region
tensors, detection records, multi context, CLI) are bit-identical to the existing RGB entries fed the reference's conversion of the
same frames.  The expected side is always an RGB entry on yuyvref.formula(), which tests/test_yuyv_host.py pins to the compiled
reference's output (tests/golden/yuyv.npz) - never the code under test."""
import json
import os
import subprocess

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv, synth
from yuyvref import formula, rgb_to_yuyv

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "yuyv.npz"))
YUYV = hipdrv.PIXFMTS["yuyv"]


def _natural(w, h):
    """the dog picture resampled to w x h (nearest), as a YUYV frame"""
    ys, xs = np.arange(h) * DOG.shape[0] // h, np.arange(w) * DOG.shape[1] // w
    return rgb_to_yuyv(DOG[ys][:, xs])


def _random(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 2), dtype=np.uint8)


def _mixed_set():
    """YUYV frames of mixed sizes: natural, random bytes (all clamps), the fixture's, a fitted height of 1, very wide"""
    return [_natural(768, 576), _random(640, 480, 1), _natural(320, 240), GOLD["random_32x24/yuyv"], GOLD["dog_64x48/yuyv"],
            _natural(300, 700), _random(300, 2, 2), _natural(1280, 720), GOLD["random_2x2/yuyv"]]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def model():
    return synth.SynthModel(seed=1, obj_bias=2.0)


def test_fixture_frames_letterbox_like_the_reference_rgb():
    """the stored reference RGB itself as the expected side"""
    for name in ("random_32x24", "random_2x1", "random_2x2", "random_6x5", "dog_64x48"):
        got = hipdrv.letterbox_pix(GOLD[name + "/yuyv"], "yuyv")
        assert _same_bits(got, hipdrv.letterbox_u8(GOLD[name + "/rgb"])), name


@pytest.mark.parametrize("w,h", [(2, 2), (6, 1000), (416, 416), (640, 480), (1280, 720), (1920, 1080)])
def test_letterbox_pix_yuyv_bit_identical_to_letterbox_u8_of_the_converted_rgb(w, h):
    for frame in (_random(w, h, w + h), _natural(w, h)):
        got = hipdrv.letterbox_pix(frame, "yuyv")
        want = hipdrv.letterbox_u8(formula(frame))
        assert _same_bits(got, want), (w, h)
    # the other two formats run the existing kernel
    rgb = formula(frame)
    assert _same_bits(hipdrv.letterbox_pix(rgb, "rgb24"), hipdrv.letterbox_u8(rgb))
    assert _same_bits(hipdrv.letterbox_pix(rgb[:, :, 1], "grey8"), hipdrv.letterbox_u8(rgb[:, :, 1].copy()))


def test_int16_region_equals_the_rgb_entry(model):
    frames = _mixed_set()
    rgb = [formula(f) for f in frames]
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(model)
    for batch, n in ((1, 3), (3, len(frames)), (64, 70)):     # 70 at batch 64: a ragged second chunk
        sel = [k % len(frames) for k in range(n)]
        got, q = ctx.run_images_host([frames[k] for k in sel], batch, pixfmt="yuyv")
        want, qw = ctx.run_images_host([rgb[k] for k in sel], batch)
        assert q == qw
        assert np.array_equal(got, want), batch
    # RGB24 / GREY8 through the new entry: exactly the old entry
    got, q = ctx.run_images_host(rgb[:4], 3, pixfmt="rgb24")
    want, qw = ctx.run_images_host(rgb[:4], 3)
    assert q == qw and np.array_equal(got, want)
    grey = [np.ascontiguousarray(im[:, :, 1]) for im in rgb[:4]]
    got, q = ctx.run_images_host(grey, 3, pixfmt="grey8")
    want, qw = ctx.run_images_host(grey, 3)
    assert q == qw and np.array_equal(got, want)
    ctx.close()


@pytest.mark.parametrize("split", [0, 1])
def test_f16_region_bitwise_equals_the_rgb_entry(model, split):
    frames = _mixed_set()
    rgb = [formula(f) for f in frames]
    tag = "<split>" if split else ""
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    for batch, n in ((1, 2), (3, len(frames)), (64, 70)):     # 64: two lanes of 32; 70 images = a ragged second chunk
        sel = [k % len(frames) for k in range(n)]
        got = ctx.run_images_f16_host([frames[k] for k in sel], batch, split=bool(split), pixfmt="yuyv")
        assert ctx.images_layer0_kernel(split) == "k_conv0_pool_mfma_yuyv" + tag
        want = ctx.run_images_f16_host([rgb[k] for k in sel], batch, split=bool(split))
        assert ctx.images_layer0_kernel(split) == "k_conv0_pool_mfma_u8" + tag      # after an RGB call: the byte kernel again
        assert _same_bits(got, want), (split, batch)
    got = ctx.run_images_f16_host(rgb[:4], 3, split=bool(split), pixfmt="rgb24")
    assert ctx.images_layer0_kernel(split) == "k_conv0_pool_mfma_u8" + tag
    assert _same_bits(got, ctx.run_images_f16_host(rgb[:4], 3, split=bool(split)))
    grey = [np.ascontiguousarray(im[:, :, 1]) for im in rgb[:4]]
    assert _same_bits(ctx.run_images_f16_host(grey, 3, split=bool(split), pixfmt="grey8"), ctx.run_images_f16_host(grey, 3, split=bool(split)))
    ctx.close()


@pytest.mark.parametrize("split", [0, 1])
def test_f16_no_mfma0_takes_the_yuyv_letterbox_route(model, split):
    frames = _mixed_set()
    rgb = [formula(f) for f in frames]
    ctx = hipdrv.Yolo2Hip(0)
    ctx.set_option("f16_no_mfma0", 1)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    got = ctx.run_images_f16_host(frames, 3, split=bool(split), pixfmt="yuyv")
    frame_kernel = "k_conv0_pool_f16<split>" if split else "k_conv0_pool_f16"
    assert ctx.images_layer0_kernel(split) == "k_letterbox_yuyv_batch + " + frame_kernel
    want = ctx.run_images_f16_host(rgb, 3, split=bool(split))
    assert ctx.images_layer0_kernel(split) == "k_letterbox_u8_batch + " + frame_kernel
    assert _same_bits(got, want)
    ctx.close()


def _same_records(a, b, n):
    assert np.array_equal(a["counts"], b["counts"])
    for f in range(n):
        assert np.array_equal(a["dets"][f], b["dets"][f]), f
    assert a["final_q"] == b["final_q"]


@pytest.mark.parametrize("precision", ["int16", "fp16", "fp32fast"])
def test_records_equal_the_rgb_entries(model, precision):
    frames = _mixed_set()[:7]
    rgb = [formula(f) for f in frames]
    thresh, nms = 0.05, 0.45
    ctx = hipdrv.Yolo2Hip(0)
    if precision == "int16":
        ctx.load_model(model)
    else:
        ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    total = 0
    for batch, best in ((3, True), (2, False)):      # 7 frames: a ragged last chunk either way
        want = hipdrv.run_images_dets(ctx._h, rgb, batch, thresh, nms, cap=4096, best_class=best, precision=precision)
        got = hipdrv.run_images_dets(ctx._h, frames, batch, thresh, nms, cap=4096, best_class=best, precision=precision, pixfmt="yuyv")
        _same_records(got, want, len(frames))
        total += int(want["counts"].sum())
    assert total > 10
    same = hipdrv.run_images_dets(ctx._h, rgb, 3, thresh, nms, cap=4096, precision=precision, pixfmt="rgb24")
    _same_records(same, hipdrv.run_images_dets(ctx._h, rgb, 3, thresh, nms, cap=4096, precision=precision), len(rgb))
    single = hipdrv.run_images_dets(ctx._h, rgb, 2, thresh, nms, cap=845, precision=precision)
    ctx.close()
    m = hipdrv.Yolo2HipMulti([0, 0])
    if precision == "int16":
        m.load_model(model)
        region, q = m.run_images(frames, 2, pixfmt="yuyv")
        region_rgb, q_rgb = m.run_images(rgb, 2)
        assert q == q_rgb and np.array_equal(region, region_rgb)
    else:
        m.load_model_fp32(model)
    gm = hipdrv.run_images_dets(m._m, frames, 2, thresh, nms, cap=845, multi=True, precision=precision, pixfmt="yuyv")
    m.close()
    _same_records(gm, single, len(frames))
    for f in range(len(frames)):
        assert (gm["dets"][f]["frame"] == f).all()


def test_pix_entries_refuse_bad_arguments_and_launch_nothing(model):
    L = hipdrv.lib()
    C = hipdrv.C
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(model)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    good = _natural(64, 48)
    n, ptrs, ws, hs, fmt, keep = hipdrv._image_args([good, good], "yuyv")
    assert fmt == YUYV
    odd = (C.c_int * 2)(64, 63)
    null_img = (C.c_void_p * 2)(ptrs[0], None)
    reg16 = np.zeros((2, 425, 13, 13), dtype=np.int16)
    regf = np.zeros((2, 425, 13, 13), dtype=np.float32)
    dets = np.zeros((2, 8), dtype=hipdrv.DET_DTYPE)
    counts = np.zeros(2, dtype=np.int32)
    q = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    entries = {
        "host": lambda p, w, f, nn: L.yolo2_hip_run_images_pix_host(ctx._h, p, w, hs, f, nn, 1, vp(reg16), C.byref(q)),
        "dets": lambda p, w, f, nn: L.yolo2_hip_run_images_pix_dets(ctx._h, p, w, hs, f, nn, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts), C.byref(q)),
        "f16_host": lambda p, w, f, nn: L.yolo2_hip_run_images_pix_f16_host(ctx._h, 0, p, w, hs, f, nn, 1, vp(regf)),
        "dets_f16": lambda p, w, f, nn: L.yolo2_hip_run_images_pix_dets_f16(ctx._h, 1, p, w, hs, f, nn, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts)),
    }
    for name, call in entries.items():
        for args, text in (((ptrs, odd, YUYV, n), b"even width, not 63"), ((ptrs, ws, 2, n), b"unknown pixel format"),
                           ((ptrs, ws, 0x59565955, n), b"unknown pixel format"), ((null_img, ws, YUYV, n), b"null image 1"),
                           ((None, ws, YUYV, n), b"null"), ((ptrs, ws, YUYV, 0), b"image count"), ((ptrs, ws, YUYV, -1), b"image count")):
            assert call(*args) == hipdrv.YOLO2_ERROR, (name, text)
            assert text in L.yolo2_hip_last_error(), (name, text, L.yolo2_hip_last_error())
    assert ctx.images_layer0_kernel(0) == "" and ctx.images_layer0_kernel(1) == ""      # no fp16 pass ran
    assert not reg16.any() and not regf.any() and not counts.any()
    # an unaligned YUYV image for the standalone letterbox; channels == 2 on the existing entries
    buf = hipdrv.DevBuf(np.zeros(64 * 48 * 2 + 8, dtype=np.uint8))
    out = hipdrv.DevBuf(np.zeros(3 * 416 * 416, dtype=np.float32))
    assert L.yolo2_hip_letterbox_pix(buf.addr + 2, 64, 48, YUYV, out.addr, 416, 416, None) == hipdrv.YOLO2_ERROR
    assert b"4-byte boundary" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_letterbox_pix(0, 64, 48, YUYV, out.addr, 416, 416, None) == hipdrv.YOLO2_ERROR
    buf.free()
    out.free()
    assert L.yolo2_hip_run_images_u8_host(ctx._h, ptrs, ws, hs, 2, n, 1, vp(reg16), C.byref(q)) == hipdrv.YOLO2_ERROR
    assert b"geometry" in L.yolo2_hip_last_error()
    # the context still works after the refusals
    got, _ = ctx.run_images_host([good], 1, pixfmt="yuyv")
    want, _ = ctx.run_images_host([formula(good)], 1)
    assert np.array_equal(got, want)
    ctx.close()


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_yuyv_stream_gives_the_rgb_streams_records(model, tmp_path):
    """7 raw YUYV frames with --video-pix-fmt yuyv422 against the RGB24 file of the converted frames: the same JSONL"""
    w, h = 320, 240
    base = _natural(w, h)
    frames = [np.ascontiguousarray(np.roll(base, 14 * k, axis=1)) for k in range(6)] + [_random(w, h, 9)]
    (tmp_path / "video.yuv").write_bytes(b"".join(f.tobytes() for f in frames) + b"\x00" * 100)      # a trailing partial frame is dropped
    (tmp_path / "video.rgb").write_bytes(b"".join(formula(f).tobytes() for f in frames))
    model.write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    size = ["--video-width", str(w), "--video-height", str(h)]
    dets = 0
    for tag, extra in (("i16", ["--precision", "int16"]), ("i16host", ["--precision", "int16", "--post", "host"]), ("f16", ["--precision", "fp16"]),
                       ("tol_multi", ["--precision", "fp32fast", "--devices", "0,0"])):
        common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.1", "--chunk-batches", "1"] + extra + size
        out = {}
        for fmt, spelled in (("rgb", "rgb24"), ("yuv", "yuyv" if tag == "f16" else "yuyv422")):
            path = tmp_path / f"{tag}_{fmt}.jsonl"
            r = _cli(common + ["--video-raw", str(tmp_path / f"video.{fmt}"), "--video-pix-fmt", spelled, "--jsonl", str(path)], tmp_path)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "Streaming inference completed successfully (7 inference frames" in r.stdout
            out[fmt] = [json.loads(line) for line in path.read_text().splitlines()]
        assert len(out["yuv"]) == 7
        for a, b in zip(out["yuv"], out["rgb"]):
            assert a.pop("source").endswith("video.yuv") and b.pop("source").endswith("video.rgb")
            assert a == b, tag
            dets += len(a["detections"])
    assert dets > 10
    # the default format is RGB24, and an annotated YUYV frame is written from converted pixels
    r = _cli(["--weights", str(tmp_path / "weights"), "--batch", "3", "--max-frames", "1", "--video-raw", str(tmp_path / "video.yuv"),
              "--video-pix-fmt", "yuyv422", "--save-annotated-dir", str(tmp_path / "ann")] + size, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ppm = (tmp_path / "ann" / "frame_000001.ppm").read_bytes()
    assert len(ppm) > w * h * 3
