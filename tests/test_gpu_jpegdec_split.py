"""Option jpegdec_split on the GPU: k_jpegdec_split (many lanes per restart interval) and k_jpegdec_rest behind
yolo2_hip_decode_jpeg_host and yolo2_hip_run_images_jpeg_dets.  Expected side: the host decoder's bytes, and the same call with the
option unset for status words and records (tests/test_gpu_jpegdec.py holds that route).  Byte / bit equality everywhere."""
import json
import os
import subprocess

import numpy as np
import pytest

import jpegdec_cases as jc
import orclib
from jpegsplit_cases import noise_streams
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu

ACCEPTED = [n for n in jc.JPEGS if hipdrv.jpeg_probe(jc.stream(n))["gpu_decodable"]]
ALL = 845 * 80


@pytest.fixture(scope="module")
def ctx():
    c = hipdrv.Yolo2Hip(0)
    yield c
    c.close()


@pytest.fixture
def split(ctx):
    """sets the option for one test and clears it behind it"""
    def use(value):
        ctx.set_option("jpegdec_split", value)
    yield use
    ctx.set_option("jpegdec_split", None)


@pytest.mark.parametrize("S", [32, 128])
def test_fixtures_in_mixed_chunks(ctx, split, S):
    """all accepted fixtures and the noise streams, batch 7: a long 4:4:4 segment over several wavefronts (jpg/base_444), more
    subsequences than a workgroup has threads (jpg/big_420), many short segments in one workgroup with some too short to split
    (jpg/restart_blocks), the slow synchroniser (jpg/base_420_q100), one component (jpg/grey)"""
    names = ACCEPTED + [f"noise{k}" for k in range(8)]
    streams = [jc.stream(n) for n in ACCEPTED] + list(noise_streams())
    if S == 32:
        shape = {n: hipdrv.jpeg_decode_ref(jc.stream(n), split=32)[2] for n in ("jpg/base_444", "jpg/big_420", "jpg/restart_blocks", "jpg/base_420_q100")}
        assert shape["jpg/base_444"]["subsequences"] > 4 * 64 - 64
        assert shape["jpg/big_420"]["subsequences"] > 1024
        assert shape["jpg/restart_blocks"]["split_segments"] > 8
        assert shape["jpg/base_420_q100"]["max_rounds"] > 100
    else:
        assert hipdrv.jpeg_decode_ref(jc.stream("jpg/restart_blocks"), split=128)[2]["short_segments"] > 0
    split(S)
    got, status = ctx.jpeg_decode(streams, batch=7)
    info = hipdrv.jpeg_split_info(ctx._h)
    assert not status.any(), dict(zip(names, status))
    for n, s, g in zip(names, streams, got):
        want = jc.host_decode(s)
        assert g.shape == want.shape and np.array_equal(g, want), f"{n}: {(g != want).sum()} bytes differ"
    assert info["split_bytes"] == S and info["split_segments"] > 0 and info["fallback_segments"] == 0 and info["short_segments"] > 0, info
    # the doorway's counts, stream by stream, are the device's
    ref = [hipdrv.jpeg_decode_ref(s, split=S)[2] for s in streams]
    for key in ("subsequences", "split_segments", "short_segments"):
        assert info[key] == sum(r[key] for r in ref), (key, info)
    assert info["max_rounds"] == max(r["max_rounds"] for r in ref), info


def test_mixed_chunk_with_damage_equals_the_call_without_the_option(ctx, split):
    """DRI and no DRI, three table sets, a copy the scan flags and a copy that decodes after falling back, in one chunk"""
    damaged = jc.damaged()
    flagged, fallen = damaged["jpg/restart_rows:rst_removed"], None
    for label, data in sorted(damaged.items()):
        if hipdrv.jpeg_probe(data)["gpu_decodable"]:
            _, st, info = hipdrv.jpeg_decode_ref(data, split=32)
            if st == 0 and info["fallback_segments"]:
                fallen = data
                break
    assert fallen is not None and hipdrv.jpeg_decode_ref(flagged)[1] == 3
    tables = [jc.write_jpg(np.random.default_rng(40 + k).integers(0, 256, (40 + k, 50 - k, 3), dtype=np.uint8), q) for k, q in enumerate((5, 80, 100))]
    streams = [jc.stream("ref/dog.jpg"), flagged, jc.stream("jpg/base_444")] + tables + [fallen, jc.stream("jpg/restart_rows")]
    want, want_status = ctx.jpeg_decode(streams, batch=len(streams), strict=False)
    assert hipdrv.jpeg_split_info(ctx._h)["subsequences"] == 0
    split(32)
    got, status = ctx.jpeg_decode(streams, batch=len(streams), strict=False)
    info = hipdrv.jpeg_split_info(ctx._h)
    assert list(status) == list(want_status) and list(status) == [0, 3, 0, 0, 0, 0, 0, 0]
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), i
        assert (not g.any()) if status[i] else np.array_equal(g, jc.host_decode(streams[i])), i
    assert info["fallback_segments"] >= 1 and info["split_segments"] > 0, info


@pytest.fixture(scope="module")
def netw():
    class Net:
        pass
    n = Net()
    model = synth.SynthModel(seed=1)
    n.ctx = hipdrv.Yolo2Hip(0)
    n.ctx.load_model(model)
    n.ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    raw = np.ascontiguousarray(jc.host_decode_fixture("jpg/base_422"))
    n.mixed = [jc.stream("ref/dog.jpg"), jc.stream("jpg/base_444"), raw, jc.stream("jpg/big_420"), jc.stream("jpg/grey")]
    yield n
    n.ctx.close()


@pytest.mark.parametrize("precision", ["int16", "fp16"])
def test_records_equal_the_call_without_the_option(netw, precision):
    """batch 3, a raw frame (sizes[i] == 0) in the first chunk"""
    run = lambda: netw.ctx.run_jpegs_dets(netw.mixed, precision=precision, batch=3, thresh=0.005, nms=0.45, cap=ALL, best_class=False)
    want = run()
    assert hipdrv.jpeg_split_info(netw.ctx._h)["subsequences"] == 0
    netw.ctx.set_option("jpegdec_split", 64)
    try:
        got = run()
        info = hipdrv.jpeg_split_info(netw.ctx._h)
    finally:
        netw.ctx.set_option("jpegdec_split", None)
    assert info["split_segments"] > 0 and info["fallback_segments"] == 0, info
    assert not got["status"].any() and want["counts"].max() > 0
    assert got["final_q"] == want["final_q"] and np.array_equal(got["counts"], want["counts"])
    for f in range(len(netw.mixed)):
        assert got["dets"][f].tobytes() == want["dets"][f].tobytes(), (precision, f)


def test_unset_option_takes_the_old_route(ctx, split):
    streams = [jc.stream("jpg/base_444"), jc.stream("jpg/restart_rows")]
    split(64)
    ctx.jpeg_decode(streams, batch=2)
    assert hipdrv.jpeg_split_info(ctx._h)["subsequences"] > 0
    ctx.set_option("jpegdec_split", None)
    ctx.jpeg_decode(streams, batch=2)
    assert hipdrv.jpeg_split_info(ctx._h) == dict(subsequences=0, split_segments=0, fallback_segments=0, short_segments=0, max_rounds=0,
                                                 split_bytes=0, split_ms=0.0, fallback_ms=0.0)
    split(0)                                                                   # 0 is "unset" too
    ctx.jpeg_decode(streams, batch=2)
    assert hipdrv.jpeg_split_info(ctx._h)["subsequences"] == 0


def test_buffers_grow_once_and_are_all_freed():
    base = hipdrv.live_bytes()
    c = hipdrv.Yolo2Hip(0)
    streams = [jc.stream("jpg/base_420"), jc.stream("jpg/restart_blocks")]
    c.jpeg_decode(streams, batch=2)
    plain = hipdrv.live_bytes()
    c.set_option("jpegdec_split", 32)
    got, status = c.jpeg_decode(streams, batch=2)
    first = hipdrv.live_bytes()
    assert not status.any() and np.array_equal(got[1], jc.host_decode_fixture("jpg/restart_blocks"))
    assert first[0] > plain[0] and first[1] > plain[1]                        # the workgroup tables and the segments' words
    c.jpeg_decode(streams, batch=2)
    assert hipdrv.live_bytes() == first                                        # a second call allocates nothing
    c.close()
    assert hipdrv.live_bytes() == base


PKG = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")


def _cli(args, cwd):
    return subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                           os.path.join(PKG, "config", "coco.names")] + args, capture_output=True, text=True, cwd=str(cwd),
                          env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_decode_split_gives_the_jsonl_of_decode_host(tmp_path):
    synth.SynthModel(seed=1).write_files(str(tmp_path / "weights"), fp32=True, int16=True)
    idir = tmp_path / "imgs"
    idir.mkdir()
    for name, data in {"00_dog.jpg": jc.stream("ref/dog.jpg"), "01_444.jpg": jc.stream("jpg/base_444"), "02_prog.jpg": jc.stream("jpg/prog_420"),
                       "03_flagged.jpg": jc.damaged()["jpg/restart_rows:stray_eoi"], "04_big.jpg": jc.stream("jpg/big_420")}.items():
        (idir / name).write_bytes(data)
    common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.005", "--chunk-batches", "1", "--precision", "int16",
              "--input-dir", str(idir)]
    out = {}
    for tag, extra in (("host", ["--decode", "host"]), ("split", ["--decode", "gpu", "--decode-split", "128"])):
        path = tmp_path / f"{tag}.jsonl"
        r = _cli(common + extra + ["--jsonl", str(path)], tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[tag] = path.read_text()
    assert out["split"] == out["host"]
    recs = [json.loads(line) for line in out["split"].splitlines()]
    assert len(recs) == 5 and sum(len(r["detections"]) for r in recs) > 0
    r = _cli(common + ["--decode-split", "128"], tmp_path)
    assert r.returncode != 0 and "--decode gpu" in r.stderr
    r = _cli(common + ["--decode", "gpu", "--decode-split", "100"], tmp_path)
    assert r.returncode != 0 and "multiple of 16" in r.stderr
