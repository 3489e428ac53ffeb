"""GPU test of the streaming CLI on the matrix-core passes: yolov2_detect --precision fp16 / fp32fast --input-dir runs the images ->
records entry yolo2_hip_run_images_u8_dets_f16 per device lane; its JSONL records equal the library's best-class records on the same
decoded images (the fixture files of tests/golden/images.npz, decoded by the project's codec to the bytes stored beside them)."""
import json
import os
import subprocess

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
PKG = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
IMAGES = np.load(os.path.join(orclib.ROOT, "tests", "golden", "images.npz"))
NAMES = ["jpg/base_444", "jpg/base_420", "jpg/base_420_narrow", "jpg/grey", "jpg/prog_422", "jpg/cmyk", "jpg/big_420", "jpg/base_1x1",
         "png/rgb", "png/rgba", "png/palette", "png/rgb_level9", "png/grey16_interlaced"]
THRESH, NMS = 0.1, 0.45


def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_f16")
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    model.write_files(str(tmp / "weights"), fp32=True, int16=False)
    idir = tmp / "imgs"
    idir.mkdir()
    for k, name in enumerate(NAMES):     # --input-dir reads a directory sorted by name: the index keeps NAMES' order
        (idir / f"{k:02d}_{name.replace('/', '_')}.{name.split('/')[0]}").write_bytes(IMAGES[name + "/file"].tobytes())
    return tmp, model, idir


@pytest.mark.parametrize("precision", ["fp16", "fp32fast"])
def test_cli_streams_images_on_the_f16_passes(setup, precision):
    tmp, model, idir = setup
    out = tmp / f"{precision}.jsonl"
    r = _cli(["--weights", str(tmp / "weights"), "--precision", precision, "--input-dir", str(idir), "--devices", "0,0", "--batch", "3",
              "--thresh", str(THRESH), "--nms", str(NMS), "--jsonl", str(out)], tmp)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"Streaming inference completed successfully ({len(NAMES)} inference frames" in r.stdout
    recs = [json.loads(line) for line in out.read_text().splitlines()]
    assert len(recs) == len(NAMES)
    imgs = [IMAGES[name + "/rgb"] for name in NAMES]
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    lib = hipdrv.run_images_dets(ctx._h, imgs, 3, THRESH, NMS, cap=845, best_class=True, precision=precision)
    ctx.close()
    total = 0
    for k, rec in enumerate(recs):
        assert (rec["width"], rec["height"]) == (imgs[k].shape[1], imgs[k].shape[0])
        want = [d for d in lib["dets"][k] if d["prob"] > THRESH]
        got = rec["detections"]
        assert len(got) == len(want), (precision, k)
        for g, w in zip(got, want):
            assert g["class_id"] == int(w["cls"])
            assert g["prob"] == float("%.6f" % w["prob"])
            assert [g["bbox_norm"][c] for c in "xywh"] == [float("%.6f" % w[c]) for c in "xywh"]
        total += len(got)
    assert total > 10


def test_cli_f16_refuses_the_host_tail(setup):
    tmp, _, idir = setup
    r = _cli(["--weights", str(tmp / "weights"), "--precision", "fp16", "--input-dir", str(idir), "--post", "host", "--jsonl",
              str(tmp / "host.jsonl")], tmp)
    assert r.returncode != 0
    assert "--post host runs the int16 region tensor only" in r.stderr
