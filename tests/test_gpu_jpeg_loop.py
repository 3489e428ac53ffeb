"""GPU tests of the camera loop from JPEG streams: yolo2_hip_loop_images_jpeg, yolo2_hip_multi_loop_images_jpeg and
yolo2_hip_multi_run_images_jpeg_dets.  Expected side everywhere: the host decoder (jpegdec_cases.host_decode, pinned to stb_image by
tests/test_host_codec.py) followed by yolo2_hip_loop_images_pix on its RGB24 frames (pinned by tests/test_gpu_loop.py), or the
single-context entry for the multi forms.  Byte equality of every output."""
import json
import os
import subprocess

import numpy as np
import pytest

import jpegdec_cases as jc
import jpegsplit_cases as js
import orclib
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
PKG = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")
NAMES = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
# ref/dog.jpg and ref/person.jpg are the h1v2 fixtures (luma 1 x 2)
SEVEN = ["jpg/base_420", "jpg/restart_rows", "jpg/grey", "jpg/base_422", "jpg/big_420", "ref/person.jpg", "ref/dog.jpg"]
THRESH, NMS, BATCH = 0.005, 0.45, 3
L = hipdrv.lib


@pytest.fixture(scope="module")
def ctx():
    model = synth.SynthModel(seed=1)
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    yield c
    c.close()


def frames_of(names):
    return [np.ascontiguousarray(jc.host_decode_fixture(n)) for n in names]


def kw(precision="int16", quality=None, tail="app", batch=BATCH):
    return dict(precision=precision, tail=tail, thresh=THRESH, nms=NMS, labels=NAMES, jpeg_quality=quality, batch=batch)


def assert_same(got, want, frames=None, shift=None):
    """every output of a loop call against another's; frames: which of `got` to compare with want's 0.. (default: all, in order)"""
    idx = list(range(len(want["frames"]))) if frames is None else frames
    assert got["final_q"] == want["final_q"]
    for w, g in enumerate(idx):
        assert got["counts"][g] == want["counts"][w] and got["drawn"][g] == want["drawn"][w], (g, w)
        exp = want["dets"][w].copy()
        exp["frame"] = g
        assert got["dets"][g].tobytes() == exp.tobytes(), g
        a, b = got["frames"][g], want["frames"][w]
        assert a is not None and (a == b if isinstance(b, bytes) else (a.shape == b.shape and np.array_equal(a, b))), g


# ------------------------------------------------------------------ 1. identity

@pytest.mark.parametrize("precision,quality", [("int16", None), ("int16", 80), ("fp16", None), ("fp16", 80), ("fp32fast", 80)])
def test_every_output_equals_host_decode_then_the_pix_loop(ctx, precision, quality):
    streams = [jc.stream(n) for n in SEVEN]
    want = ctx.loop_images(frames_of(SEVEN), pixfmt="rgb24", **kw(precision, quality))
    assert want["counts"].max() > 0 and want["drawn"].max() > 0          # records exist and are drawn
    got = ctx.loop_jpegs(streams, **kw(precision, quality))
    assert not got["status"].any()
    assert got["sizes"] == [(f.shape[1], f.shape[0]) for f in frames_of(SEVEN)]
    assert_same(got, want)
    j = hipdrv.jpeg_last_info(ctx._h)
    assert j["frames"] == 7 and j["chunks"] == 3 and ctx.loop_last_info()["chunks"] == 3


# ------------------------------------------------------------------ 2. option jpegdec_split

@pytest.mark.parametrize("precision,quality", [("int16", 80), ("fp16", None)])
def test_split_option_changes_nothing_but_the_launches(ctx, precision, quality):
    names = ["jpg/big_420", "ref/person.jpg", "jpg/base_420", "jpg/restart_rows"]      # no DRI, DRI 80, no DRI (short), DRI 13
    assert [hipdrv.jpeg_probe(jc.stream(n))["restart_interval"] for n in names[:2]] == [0, 80]
    streams = [jc.stream(n) for n in names] + [js.noise_streams()[3]]
    want = ctx.loop_images(frames_of(names) + [jc.host_decode(streams[-1])], pixfmt="rgb24", **kw(precision, quality))
    ctx.set_option("jpegdec_split", "64")
    try:
        got = ctx.loop_jpegs(streams, **kw(precision, quality))
        info = hipdrv.jpeg_split_info(ctx._h)
    finally:
        ctx.set_option("jpegdec_split", None)
    assert info["split_bytes"] == 64 and info["split_segments"] > 0, info
    assert not got["status"].any() and want["drawn"].max() > 0
    assert_same(got, want)
    assert_same(ctx.loop_jpegs(streams, **kw(precision, quality)), want)
    assert hipdrv.jpeg_split_info(ctx._h)["split_segments"] == 0               # read per call: unset again


# ------------------------------------------------------------------ 3. raw frames mixed in

def test_host_decoded_frames_ride_along_as_raw_frames(ctx):
    names = ["jpg/base_420", "jpg/prog_420", "jpg/grey", "jpg/cmyk", "ref/person.jpg"]
    frames = frames_of(names)
    mixed = [frames[i] if n in ("jpg/prog_420", "jpg/cmyk") else jc.stream(n) for i, n in enumerate(names)]
    for quality in (None, 80):
        want = ctx.loop_images(frames, pixfmt="rgb24", **kw("int16", quality, batch=2))
        got = ctx.loop_jpegs(mixed, **kw("int16", quality, batch=2))
        assert not got["status"].any() and want["drawn"].max() > 0
        assert_same(got, want)
    info, j = ctx.loop_last_info(), hipdrv.jpeg_last_info(ctx._h)
    raw = frames[1].size + frames[3].size
    assert info["image_bytes_staged"] == raw + sum(len(s) for s in mixed if isinstance(s, bytes))
    assert info["image_bytes_h2d"] == j["stream_bytes_h2d"] + j["frame_bytes_h2d"] and j["frame_bytes_h2d"] > raw


# ------------------------------------------------------------------ 4. a flagged frame

@pytest.mark.parametrize("quality", [None, 80])
def test_flagged_frame_returns_nothing_and_its_neighbours_are_complete(ctx, quality):
    names = ["jpg/base_420", "ref/person.jpg", "jpg/big_420", "jpg/grey"]
    bad = jc.damaged()["jpg/restart_rows:stray_eoi"]
    assert hipdrv.jpeg_decode_ref(bad)[1] != 0
    streams = [jc.stream(n) for n in names]
    streams.insert(2, bad)
    want = ctx.loop_jpegs([jc.stream(n) for n in names], **kw("int16", quality))
    assert want["drawn"].max() > 0
    with pytest.raises(hipdrv.Yolo2HipError, match="frame 2: the GPU decoder flagged"):
        ctx.loop_jpegs(streams, **kw("int16", quality))
    got = ctx.loop_jpegs(streams, strict=False, **kw("int16", quality))
    assert [bool(s) for s in got["status"]] == [False, False, True, False, False]
    assert got["counts"][2] == 0 and got["drawn"][2] == 0 and got["frames"][2] is None and len(got["dets"][2]) == 0
    assert_same(got, want, frames=[0, 1, 3, 4])
    # the raw entry: nothing is written to out[2], its size is 0
    caps = [hipdrv.jpeg_bound(97, 61) if quality else 97 * 61 * 3] * 3
    rc, dets, counts, q, outs, sizes, drawn, status, ws, hs = hipdrv.loop_jpegs_raw(
        ctx._h, [streams[0], bad, streams[0]], 0, hipdrv.DETS_BEST_CLASS, THRESH, NMS, 3, 845, NAMES, int(bool(quality)), quality or 0, caps, guard=16)
    assert rc == hipdrv.YOLO2_ERROR and b"frame 1: the GPU decoder flagged" in L().yolo2_hip_last_error()
    assert status[1] != 0 and counts[1] == 0 and drawn[1] == 0 and sizes[1] == 0 and (outs[1] == 0xA5).all()
    assert sizes[0] == sizes[2] > 0 and outs[0][:int(sizes[0])].tobytes() == outs[2][:int(sizes[2])].tobytes()
    assert all((o[int(c):] == 0xA5).all() for o, c in zip(outs, caps))         # nothing past any buffer's capacity


# ------------------------------------------------------------------ 5. refusals

def test_refusals_come_before_any_launch_and_touch_nothing(ctx):
    ok, prog = jc.stream("jpg/base_420"), jc.stream("jpg/prog_420")
    held = hipdrv.live_bytes()

    def raw(streams, caps, precision=0, flags=hipdrv.DETS_BEST_CLASS, out_format=0, quality=0):
        return hipdrv.loop_jpegs_raw(ctx._h, streams, precision, flags, THRESH, NMS, 2, 845, NAMES, out_format, quality, caps, guard=8)

    def untouched(r):
        rc, dets, counts, q, outs, sizes, drawn, status, ws, hs = r
        assert all((o == 0xA5).all() for o in outs) and (dets.view(np.uint8) == 0xA5).all()
        assert (counts == -77).all() and (drawn == -77).all() and (status == -77).all() and (sizes == (1 << 40) + 7).all()
        assert (np.asarray(ws) == -77).all() and (np.asarray(hs) == -77).all()
        assert hipdrv.live_bytes() == held

    full = 97 * 61 * 3
    for what, call in ((b"frame 1: not GPU-decodable (reason 2: progressive)", lambda: raw([ok, prog], [full, full])),
                       (b"frame 0: not GPU-decodable (reason 4", lambda: raw([jc.stream("jpg/cmyk"), ok], [full, full])),
                       (b"output buffer too small for frame 1 (%d < %d bytes)" % (full - 1, full), lambda: raw([ok, ok], [full, full - 1])),
                       (b"have no int8 form", lambda: raw([ok, ok], [full, full], precision=3)),
                       (b"unknown precision", lambda: raw([ok, ok], [full, full], precision=4)),
                       (b"YOLO2_DETS_BEST_CLASS", lambda: raw([ok, ok], [full, full], flags=hipdrv.DETS_APP_TAIL)),
                       (b"quality 0", lambda: raw([ok, ok], [4096, 4096], out_format=1, quality=0)),
                       (b"output format", lambda: raw([ok, ok], [full, full], out_format=2))):
        r = call()
        assert r[0] == hipdrv.YOLO2_ERROR and what in L().yolo2_hip_last_error(), (what, L().yolo2_hip_last_error())
        untouched(r)
    with pytest.raises(hipdrv.Yolo2HipError, match=r"frame 1: not GPU-decodable \(reason 2: progressive\)"):
        ctx.loop_jpegs([ok, prog], **kw())
    # a short JPEG caps[f]: the loop's rule - the call runs, reports the size needed and names the frame
    want = ctx.loop_jpegs([ok, ok], **kw("int16", 80))
    need = len(want["frames"][1])
    rc, dets, counts, q, outs, sizes, drawn, status, ws, hs = hipdrv.loop_jpegs_raw(
        ctx._h, [ok, ok], 0, hipdrv.DETS_BEST_CLASS | hipdrv.DETS_APP_TAIL, THRESH, NMS, 2, 845, NAMES, 1, 80, [need, need - 1], guard=8)
    assert rc == hipdrv.YOLO2_ERROR and b"output buffer too small for frame 1 (%d < %d bytes)" % (need - 1, need) in L().yolo2_hip_last_error()
    assert list(sizes) == [need, need] and outs[0][:need].tobytes() == want["frames"][0] and (outs[0][need:] == 0xA5).all()
    assert outs[1][:need - 1].tobytes() == want["frames"][1][:need - 1] and (outs[1][need - 1:] == 0xA5).all()
    assert not status.any() and np.array_equal(counts, want["counts"])


# ------------------------------------------------------------------ 6. what goes up

def test_only_compressed_bytes_go_up(ctx):
    dog = jc.stream("ref/dog.jpg")
    frames = [np.ascontiguousarray(jc.host_decode_fixture("ref/dog.jpg"))] * 4
    for quality in (None, 80):
        ctx.loop_images(frames, pixfmt="rgb24", **kw("fp16", quality, batch=4))
        pix = ctx.loop_last_info()
        ctx.loop_jpegs([dog] * 4, **kw("fp16", quality, batch=4))
        info, j = ctx.loop_last_info(), hipdrv.jpeg_last_info(ctx._h)
        assert info["image_bytes_staged"] == 4 * len(dog)
        assert 4 * len(dog) <= info["image_bytes_h2d"] < pix["image_bytes_h2d"]
        assert info["image_bytes_h2d"] == j["stream_bytes_h2d"] + j["frame_bytes_h2d"]
        assert info["image_bytes_h2d"] < 4 * len(dog) + 256 * 1024            # tables and descriptors beside the streams, no frame
        assert j["frames"] == 4 and j["chunks"] == 1
        assert info["out_bytes_d2h"] == pix["out_bytes_d2h"] and info["items_built"] == pix["items_built"] > 0


# ------------------------------------------------------------------ 7. neighbours on one context, 8. memory

def test_neighbouring_entries_keep_their_buffers_and_memory_balances():
    """loop_jpegs, run_jpegs_dets, loop_images, annotate_images and loop_jpegs at a larger batch on ONE context: each gives what it gives
    on a context of its own (a buffer regrown by one entry drops none a neighbour still relies on); close() gives everything back"""
    base = hipdrv.live_bytes()
    model = synth.SynthModel(seed=1)
    names = ["jpg/base_420", "jpg/grey", "ref/person.jpg", "jpg/big_420", "jpg/restart_rows"]
    streams, frames = [jc.stream(n) for n in names], frames_of(names)
    steps = [lambda c: c.loop_jpegs(streams, **kw("int16", 80, batch=2)),
             lambda c: c.run_jpegs_dets(streams, precision="int16", tail="app", batch=2, thresh=THRESH, nms=NMS),
             lambda c: c.loop_images(frames, pixfmt="rgb24", **kw("int16", None, batch=2)),
             None,                                                   # annotate_images on the records of step 1, below
             lambda c: c.loop_jpegs(streams * 2, **kw("int16", 80, batch=5))]

    def context():
        c = hipdrv.Yolo2Hip(0)
        c.load_model(model)
        return c

    solo = []
    for step in steps:
        c = context()
        solo.append(step(c) if step else c.annotate_images(frames, solo[1]["dets"], None, 2, THRESH, labels=NAMES, pixfmt="rgb24"))
        c.close()
    assert hipdrv.live_bytes() == base
    c = context()
    together = [step(c) if step else c.annotate_images(frames, solo[1]["dets"], None, 2, THRESH, labels=NAMES, pixfmt="rgb24") for step in steps]
    c.close()
    assert hipdrv.live_bytes() == base                                   # 8. everything is given back
    assert solo[0]["drawn"].max() > 0 and solo[1]["counts"].max() > 0
    for k in (0, 2, 4):
        assert_same(together[k], solo[k])
    assert np.array_equal(together[1]["counts"], solo[1]["counts"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(together[1]["dets"], solo[1]["dets"]))
    assert all(np.array_equal(a, b) for a, b in zip(together[3][0], solo[3][0])) and list(together[3][1]) == list(solo[3][1])


# ------------------------------------------------------------------ 9. the multi forms

@pytest.mark.parametrize("precision", ["int16", "fp16"])
def test_multi_forms_equal_the_single_context(ctx, precision):
    names = ["jpg/base_420", "ref/person.jpg", "jpg/grey", "jpg/big_420", "jpg/restart_rows"]
    streams = [jc.stream(n) for n in names]
    model = synth.SynthModel(seed=1)
    m = hipdrv.Yolo2HipMulti([0, 0])
    try:
        if precision == "int16":
            m.load_model(model)
        else:
            m.load_model_fp32(model)
        for quality in (None, 80):
            want = ctx.loop_jpegs(streams, **kw(precision, quality, batch=2))
            got = m.loop_jpegs(streams, batch_per_device=2, **{k: v for k, v in kw(precision, quality).items() if k != "batch"})
            assert not got["status"].any() and want["drawn"].max() > 0 and got["sizes"] == want["sizes"]
            assert_same(got, want)                                   # (frame numbers global: assert_same expects frame == index)
        want = ctx.run_jpegs_dets(streams, precision=precision, tail="app", batch=2, thresh=THRESH, nms=NMS)
        got = m.run_jpegs_dets(streams, batch_per_device=2, thresh=THRESH, nms=NMS, precision=precision, tail="app")
        assert got["final_q"] == want["final_q"] and np.array_equal(got["counts"], want["counts"]) and want["counts"].max() > 0
        assert got["sizes"] == want["sizes"] and not got["status"].any()
        for f in range(len(streams)):
            assert got["dets"][f].tobytes() == want["dets"][f].tobytes() and (got["dets"][f]["frame"] == f).all(), f
        with pytest.raises(hipdrv.Yolo2HipError, match=r"frame 3: not GPU-decodable \(reason 2: progressive\)"):
            m.loop_jpegs(streams[:3] + [jc.stream("jpg/prog_420")], batch_per_device=2, precision=precision)
        with pytest.raises(hipdrv.Yolo2HipError, match=r"frame 3: not GPU-decodable \(reason 2: progressive\)"):
            m.run_jpegs_dets(streams[:3] + [jc.stream("jpg/prog_420")], batch_per_device=2, precision=precision)
    finally:
        m.close()


# ------------------------------------------------------------------ 10. CLI

def _cli(args, cwd):
    return subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                           os.path.join(PKG, "config", "coco.names")] + args, capture_output=True, text=True, cwd=str(cwd),
                          env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_decode_gpu_with_the_loop_writes_what_decode_host_writes(tmp_path):
    """the directory of tests/test_gpu_jpegdec.py's decode test (baseline, progressive, CMYK and PNG files, two streams the GPU decoder
    flags) and a --video-mjpeg file of five streams: JSONL and every saved file of --decode gpu --decode-split 128 are --decode host's"""
    synth.SynthModel(seed=1).write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    idir = tmp_path / "imgs"
    idir.mkdir()
    files = {"00_dog.jpg": jc.stream("ref/dog.jpg"), "01_prog.jpg": jc.stream("jpg/prog_420"), "02_rgb.png": jc.IMAGES["png/rgb/file"].tobytes(),
             "03_grey.jpg": jc.stream("jpg/grey"), "04_flagged.jpg": jc.damaged()["jpg/restart_rows:stray_eoi"],
             "05_420.jpg": jc.stream("jpg/base_420"), "06_cmyk.jpg": jc.stream("jpg/cmyk"), "07_unreadable.jpg": jc.damaged()["jpg/restart_rows:rst_removed"]}
    for name, data in files.items():
        (idir / name).write_bytes(data)
    five = [jc.stream(n) for n in ("jpg/restart_rows", "ref/person.jpg", "jpg/prog_444", "jpg/base_422", "jpg/big_420")]
    (tmp_path / "cam.mjpeg").write_bytes(b"\x00junk".join(five) + b"tail")
    common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.005", "--chunk-batches", "1", "--post", "gpu", "--loop-gpu",
              "--annotate-gpu", "--annotated-format", "jpg"]
    dets = 0
    for tag, src, extra, frames in (("dir", ["--input-dir", str(idir)], ["--precision", "int16"], 7),
                                    ("mjpeg", ["--video-mjpeg", str(tmp_path / "cam.mjpeg")], ["--precision", "fp16", "--tail", "app"], 5)):
        out = {}
        for decode, more in (("host", []), ("gpu", ["--decode-split", "128"])):
            path, d = tmp_path / f"{tag}_{decode}.jsonl", tmp_path / f"{tag}_{decode}"
            r = _cli(common + extra + src + ["--decode", decode] + more + ["--jsonl", str(path), "--save-annotated-dir", str(d)], tmp_path)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Streaming inference completed successfully ({frames} inference frames" in r.stdout
            out[decode] = (path.read_text(), sorted(os.listdir(d)), [(d / n).read_bytes() for n in sorted(os.listdir(d))])
        assert out["gpu"][0] == out["host"][0], tag
        assert out["gpu"][1] == out["host"][1] and len(out["gpu"][1]) == frames, tag
        assert out["gpu"][2] == out["host"][2], tag
        dets += sum(len(json.loads(line)["detections"]) for line in out["gpu"][0].splitlines())
    assert dets > 0
