"""JPEG streams decoded on the GPU (include/yolo2_hip.h "JPEG streams decoded on the GPU"): k_jpegdec_entropy / _idct / _rgb behind
yolo2_hip_decode_jpeg_host and yolo2_hip_run_images_jpeg_dets.  Expected side: the host decoder y2h_decode_image (pinned to stb_image by
tests/test_host_codec.py), the host doorway's status (tests/test_jpegdec_host.py has checked it against the host decoder) and the
_pix_dets entries fed the host-decoded frames.  Byte / bit equality everywhere."""
import json
import os
import subprocess

import numpy as np
import pytest

import jpegdec_cases as jc
import orclib
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu

ACCEPTED = [n for n in jc.JPEGS if hipdrv.jpeg_probe(jc.stream(n))["gpu_decodable"]]


@pytest.fixture(scope="module")
def ctx():
    c = hipdrv.Yolo2Hip(0)
    yield c
    c.close()


def _assert_decodes(ctx, streams, batch, labels=None):
    got, status = ctx.jpeg_decode(streams, batch=batch)
    assert not status.any(), status
    for i, s in enumerate(streams):
        want = jc.host_decode(s)
        assert got[i].shape == want.shape, (labels[i] if labels else i, got[i].shape, want.shape)
        assert np.array_equal(got[i], want), f"{labels[i] if labels else i}: {(got[i] != want).sum()} bytes differ"


def test_fixtures_through_the_decode_entry(ctx):
    """every accepted fixture in one call at batch 8: chunks with a ragged last one, 1 x 1 to 1352 x 900, DRI and no DRI side by side"""
    assert len(ACCEPTED) >= 20 and len(ACCEPTED) % 8 != 0
    got, status = ctx.jpeg_decode([jc.stream(n) for n in ACCEPTED], batch=8)
    assert not status.any(), dict(zip(ACCEPTED, status))
    for n, g in zip(ACCEPTED, got):
        want = jc.host_decode_fixture(n)
        assert g.shape == want.shape and np.array_equal(g, want), f"{n}: {(g != want).sum()} bytes differ"


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_edge_geometry(ctx):
    sizes = [(1, 1), (9, 7), (8, 8), (8, 9), (33, 17)]                      # (h, w): 1x1, 7x9, 8x8, 9x8, 17x33
    streams = [jc.write_jpg(_noise(h, w, 10 + k), 80) for k, (h, w) in enumerate(sizes)]
    long_scan = jc.write_jpg(_noise(240, 320, 3), 100)
    scan = jc.header_facts(long_scan)["scan"]
    assert b"\xff\x00" in long_scan[scan:]                                     # stuffed bytes inside the scan
    assert _has_code_over_9_bits(long_scan), "the noise stream does not reach the slow path of Bits::symbol"
    streams += [long_scan] + [jc.stream(n) for n in ("jpg/base_420_narrow", "jpg/base_422_narrow", "jpg/base_1x1")]
    _assert_decodes(ctx, streams, batch=16)


def _has_code_over_9_bits(data: bytes) -> bool:
    """True iff the scan uses a Huffman code of more than 9 bits: a copy of the stream whose DHT lists the symbols of those codes in
    reverse order (codes of <= 9 bits untouched) must then decode differently on the host decoder, or not at all"""
    d, i, changed = bytearray(data), 2, False
    while d[i + 1] != 0xDA:
        L = (d[i + 2] << 8) | d[i + 3]
        if d[i + 1] == 0xC4:
            p = i + 4
            while p < i + 2 + L:
                counts = d[p + 1:p + 17]
                lo, hi = p + 17 + sum(counts[:9]), p + 17 + sum(counts)
                if hi - lo >= 2:
                    d[lo:hi] = d[lo:hi][::-1]
                    changed = True
                p = hi
        i += 2 + L
    other = jc.host_decode(bytes(d))
    return changed and (other is None or not np.array_equal(other, jc.host_decode(data)))


def test_more_lanes_than_a_wavefront(ctx):
    """70 frames without DRI in one chunk (one lane per frame: two wavefronts, the second partial), all from one table set"""
    rng = np.random.default_rng(5)
    sizes = [(int(rng.integers(1, 41)), int(rng.integers(1, 41))) for _ in range(70)]
    streams = [jc.write_jpg(_noise(h, w, 100 + k), 80) for k, (h, w) in enumerate(sizes)]
    _assert_decodes(ctx, streams, batch=70)


def test_restart_intervals_alone(ctx):
    _assert_decodes(ctx, [jc.stream("ref/dog.jpg")], batch=1, labels=["dog: 36 segments"])
    _assert_decodes(ctx, [jc.stream("ref/image2.jpg")], batch=1, labels=["image2: DRI 169"])


def test_three_table_sets_in_one_chunk(ctx):
    """workgroups whose lanes name different table sets read them from global memory"""
    streams = [jc.write_jpg(_noise(24 + k, 31 - k, 200 + k), (5, 80, 100)[k % 3]) for k in range(9)]
    _assert_decodes(ctx, streams + [jc.stream("jpg/restart_blocks"), jc.stream("jpg/grey")], batch=11)


def _flagged_cases():
    """damaged copies the probe accepts (the entry refuses the others before any launch) with the doorway's status"""
    out = []
    for label, data in sorted(jc.damaged().items()):
        if hipdrv.jpeg_probe(data)["gpu_decodable"]:
            out.append((label, data, hipdrv.jpeg_decode_ref(data)[1]))
    return out


def test_status_contract(ctx):
    cases = _flagged_cases()
    assert any(s for _, _, s in cases) and any(s == 0 for _, _, s in cases)
    intact = ["jpg/base_444", "jpg/restart_rows", "jpg/grey", "ref/person.jpg"]
    streams, want_status, labels = [], [], []
    for k, (label, data, st) in enumerate(cases):          # damaged and intact ones alternate
        streams += [data, jc.stream(intact[k % len(intact)])]
        want_status += [st, 0]
        labels += [label, intact[k % len(intact)]]
    got, status = ctx.jpeg_decode(streams, batch=len(streams), strict=False)
    assert list(status) == want_status, dict(zip(labels, zip(status, want_status)))
    for i, s in enumerate(streams):
        if status[i] == 0:
            want = jc.host_decode(s)
            assert got[i].shape == want.shape and np.array_equal(got[i], want), labels[i]
        else:
            assert not got[i].any(), labels[i]              # zero-filled, not a guess
    with pytest.raises(hipdrv.Yolo2HipError, match=r"frame \d+: the GPU decoder flagged"):
        ctx.jpeg_decode(streams, batch=len(streams))


# ------------------------------------------------------------------ records

ALL = 845 * 80
EIGHT = ["ref/dog.jpg", "jpg/grey", "jpg/base_420", "jpg/base_422", "jpg/restart_rows", "ref/person.jpg", "jpg/base_444", "jpg/big_420"]


@pytest.fixture(scope="module")
def netw():
    """one context with the int16, fp32 and int8 weight sets of SynthModel(seed=1); per precision the records of the matching
    _pix_dets entry on the host-decoded frames.  Computed once, shared, left unchanged."""
    class Net:
        pass
    n = Net()
    model = synth.SynthModel(seed=1)
    n.ctx = hipdrv.Yolo2Hip(0)
    n.ctx.load_model(model)
    n.ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    n.ctx.load_model(n.ctx.calibrate_int8(frames=synth.frames(40, 4), batch=4))
    n.streams = [jc.stream(name) for name in EIGHT]
    n.frames = [np.ascontiguousarray(jc.host_decode_fixture(name)) for name in EIGHT]
    # two raw frames in the middle of the chunk sequence
    n.raw = [np.random.default_rng(77).integers(0, 256, (50, 70, 3), dtype=np.uint8), n.frames[0][:200, :300].copy()]
    n.mixed = n.streams[:3] + n.raw + n.streams[3:]
    n.mixed_frames = n.frames[:3] + n.raw + n.frames[3:]
    n.thresh = 0.005
    yield n
    n.ctx.close()


@pytest.mark.parametrize("precision", ["int16", "fp16", "fp32fast", "int8"])
@pytest.mark.parametrize("tail", ["core", "app"])
def test_records_equal_the_pix_entry_on_host_decoded_frames(netw, precision, tail):
    thresh = netw.thresh
    expected = lambda: hipdrv.run_images_dets(netw.ctx._h, netw.mixed_frames, 3, thresh, 0.45, cap=ALL, best_class=False, precision=precision,
                                              pixfmt="rgb24", tail=tail)
    want = expected()
    while want["counts"].max() == 0 and thresh > 1e-6:               # (chosen on the expected side, never on the entry under test)
        thresh /= 4
        want = expected()
    assert want["counts"].max() > 0
    got = netw.ctx.run_jpegs_dets(netw.mixed, precision=precision, tail=tail, batch=3, thresh=thresh, nms=0.45, cap=ALL, best_class=False)
    assert not got["status"].any()
    assert got["final_q"] == want["final_q"] and np.array_equal(got["counts"], want["counts"])
    assert got["sizes"] == [(f.shape[1], f.shape[0]) for f in netw.mixed_frames]
    for f in range(len(netw.mixed)):
        assert got["dets"][f].tobytes() == want["dets"][f].tobytes(), (precision, tail, f)
        assert (got["dets"][f]["frame"] == f).all()


def test_flagged_frame_has_no_records_and_its_neighbours_are_complete(netw):
    bad = jc.damaged()["jpg/restart_rows:rst_removed"]
    streams = netw.streams[:2] + [bad] + netw.streams[2:4]
    want = hipdrv.run_images_dets(netw.ctx._h, netw.frames[:4], 3, netw.thresh, 0.45, cap=ALL, best_class=False, precision="int16", pixfmt="rgb24")
    with pytest.raises(hipdrv.Yolo2HipError, match="frame 2: the GPU decoder flagged"):
        netw.ctx.run_jpegs_dets(streams, batch=3, thresh=netw.thresh, cap=ALL, best_class=False)
    got = netw.ctx.run_jpegs_dets(streams, batch=3, thresh=netw.thresh, cap=ALL, best_class=False, strict=False)
    assert list(got["status"]) == [0, 0, 3, 0, 0] and got["counts"][2] == 0 and len(got["dets"][2]) == 0
    assert want["counts"].max() > 0
    for g, w in zip((0, 1, 3, 4), range(4)):
        exp = want["dets"][w].copy()
        exp["frame"] = g                                             # (frame numbers are the call's own)
        assert got["counts"][g] == want["counts"][w] and got["dets"][g].tobytes() == exp.tobytes(), g


def test_refusals_name_the_frame_and_launch_nothing(netw):
    ok = jc.stream("jpg/base_420")
    with pytest.raises(hipdrv.Yolo2HipError, match=r"frame 1: not GPU-decodable \(reason 2: progressive\)"):
        netw.ctx.jpeg_decode([ok, jc.stream("jpg/prog_420")])
    with pytest.raises(hipdrv.Yolo2HipError, match=r"frame 1: not GPU-decodable \(reason 4"):
        netw.ctx.run_jpegs_dets([ok, jc.stream("jpg/cmyk")], batch=2)
    # a short caps[i]
    C = hipdrv.C
    out = np.zeros(97 * 61 * 3 - 1, dtype=np.uint8)
    ptrs, sizes = (C.c_char_p * 1)(ok), (C.c_size_t * 1)(len(ok))
    optrs, caps = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(out.size)
    w, h, st = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    assert hipdrv.lib().yolo2_hip_decode_jpeg_host(netw.ctx._h, ptrs, sizes, 1, 1, optrs, caps, w, h, st) == hipdrv.YOLO2_ERROR
    assert "frame 0: output buffer too small" in hipdrv.lib().yolo2_hip_last_error().decode()
    assert not out.any()
    # missing weights
    bare = hipdrv.Yolo2Hip(0)
    before = hipdrv.live_bytes()
    try:
        for precision, msg in (("int16", "weights not loaded"), ("fp16", "fp32 weights not loaded"), ("int8", "int8 weights not loaded")):
            with pytest.raises(hipdrv.Yolo2HipError, match=msg):
                bare.run_jpegs_dets([ok], precision=precision, batch=1)
        assert hipdrv.live_bytes() == before                         # nothing was allocated for any of the refused calls
    finally:
        bare.close()
    with pytest.raises(hipdrv.Yolo2HipError, match="unknown precision"):
        hipdrv.check(hipdrv.lib().yolo2_hip_run_images_jpeg_dets(netw.ctx._h, 7, ptrs, sizes, w, h, 1, 1, 0.2, 0.4, 0, out.ctypes.data, 1, st, None, st),
                     "yolo2_hip_run_images_jpeg_dets")


def test_buffers_grow_and_are_all_freed():
    base = hipdrv.live_bytes()
    c = hipdrv.Yolo2Hip(0)
    small = [jc.stream("jpg/base_420"), jc.stream("jpg/restart_blocks")]
    c.jpeg_decode(small, batch=2)
    first = hipdrv.live_bytes()
    c.jpeg_decode(small, batch=2)
    assert hipdrv.live_bytes() == first                              # a second call of the same size allocates nothing
    big = small + [jc.stream("ref/dog.jpg"), jc.stream("jpg/big_420"), jc.stream("jpg/grey")]
    got, status = c.jpeg_decode(big, batch=5)
    assert not status.any() and np.array_equal(got[2], jc.host_decode_fixture("ref/dog.jpg"))
    grown = hipdrv.live_bytes()
    assert grown[0] > first[0] and grown[1] > first[1]
    c.jpeg_decode(small, batch=2)
    assert hipdrv.live_bytes() == grown                              # ... and never shrinks or leaks on the way back
    c.close()
    assert hipdrv.live_bytes() == base


# ------------------------------------------------------------------ CLI

PKG = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")


def _cli(args, cwd):
    return subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                           os.path.join(PKG, "config", "coco.names")] + args, capture_output=True, text=True, cwd=str(cwd),
                          env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_decode_gpu_gives_the_jsonl_of_decode_host(tmp_path):
    """a directory of baseline, progressive, CMYK and PNG files (and two streams the GPU decoder flags), and a --video-mjpeg file of five
    concatenated streams with bytes between them: --decode gpu writes the JSONL of --decode host"""
    synth.SynthModel(seed=1).write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    idir = tmp_path / "imgs"
    idir.mkdir()
    files = {"00_dog.jpg": jc.stream("ref/dog.jpg"), "01_prog.jpg": jc.stream("jpg/prog_420"), "02_rgb.png": jc.IMAGES["png/rgb/file"].tobytes(),
             "03_grey.jpg": jc.stream("jpg/grey"), "04_flagged.jpg": jc.damaged()["jpg/restart_rows:stray_eoi"],
             "05_420.jpg": jc.stream("jpg/base_420"), "06_cmyk.jpg": jc.stream("jpg/cmyk"), "07_unreadable.jpg": jc.damaged()["jpg/restart_rows:rst_removed"]}
    for name, data in files.items():
        (idir / name).write_bytes(data)
    # the GPU decoder flags both damaged streams; the host decoder reads the first (it is run again as a raw frame) and throws on the
    # second (it is skipped, as --decode host skips it)
    assert hipdrv.jpeg_decode_ref(files["04_flagged.jpg"])[1] == 3 and jc.host_decode(files["04_flagged.jpg"]) is not None
    assert hipdrv.jpeg_decode_ref(files["07_unreadable.jpg"])[1] == 3 and jc.host_decode(files["07_unreadable.jpg"]) is None
    five = [jc.stream(n) for n in ("jpg/restart_rows", "ref/person.jpg", "jpg/prog_444", "jpg/base_422", "jpg/big_420")]
    (tmp_path / "cam.mjpeg").write_bytes(b"\x00junk".join(five) + b"tail")
    common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.005", "--chunk-batches", "1"]
    dets = 0
    for tag, src, extra, frames in (("dir", ["--input-dir", str(idir)], ["--precision", "int16"], 7),
                                    ("mjpeg", ["--video-mjpeg", str(tmp_path / "cam.mjpeg")], ["--precision", "fp16", "--tail", "app"], 5)):
        out = {}
        for decode in ("host", "gpu"):
            path = tmp_path / f"{tag}_{decode}.jsonl"
            r = _cli(common + extra + src + ["--decode", decode, "--jsonl", str(path)], tmp_path)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Streaming inference completed successfully ({frames} inference frames" in r.stdout
            assert ("Frame 8 skipped: " in r.stdout) == (tag == "dir")
            out[decode] = path.read_text()
        assert out["gpu"] == out["host"], tag
        recs = [json.loads(line) for line in out["gpu"].splitlines()]
        assert len(recs) == frames
        dets += sum(len(r["detections"]) for r in recs)
    assert dets > 0
    r = _cli(common + ["--input-dir", str(idir), "--decode", "gpu", "--save-annotated-dir", str(tmp_path / "out")], tmp_path)
    assert r.returncode != 0 and "--decode gpu" in r.stderr
