"""GPU tests of the camera loop's detection tail (yolo2_hip_postprocess_*_app, YOLO2_DETS_APP_TAIL): bit-identical to the
reference's linux_app/src/yolo2_postprocess.c on the same int16 region tensor.  Checkers: what that file itself computed
(tests/golden/apptail.npz), the host restatement pinned to it on the CPU (tests/test_app_tail_host.py) on other tensors, and the
reference's own application (oracle/_ref/yolo2_linux) where it was built."""
import importlib.util
import json
import os
import re
import subprocess
import time

import numpy as np
import pytest

import apptail_fix as af
import orclib
from yolo2_amd import hipdrv, synth
from yuyvref import formula, rgb_to_yuyv

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
APP = os.path.join(ROOT, "oracle", "_ref", "yolo2_linux")
FULL = np.load(os.path.join(ROOT, "tests", "golden", "fullnet.npz"))
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))
REFAPP = np.load(os.path.join(ROOT, "tests", "golden", "refapp.npz"))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = hipdrv.Yolo2Hip(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", af.CASES)
def test_gpu_app_tail_equals_reference_bit_for_bit(ctx, name):
    c = af.case(name)
    t, q = af.tensor(c["tensor"])
    buf = hipdrv.DevBuf(t.copy())
    n = c["total"]
    out = hipdrv.postprocess(ctx, buf.addr, 1, [c["w"]], [c["h"]], c["thresh"], c["nms"], final_q=q, cap=8192, want_rows=True, want_proc=True,
                             tail="app")
    assert int(out["totals"][0]) == n
    assert np.array_equal(u32(out["proc"][0]), c["proc"])
    rows = out["rows"][0]
    assert np.array_equal(u32(rows[:n]), c["rows"]), "dets[] after yolo2_do_nms_sort, in its order"
    assert not rows[n:].any()
    # the records are exactly the (row, class) pairs with prob > 0, in array order
    pi, pv = af.pair_records(rows[:n])
    gi, gv = af.rec_arrays(out["dets"][0])
    assert int(out["counts"][0]) == len(pi) and np.array_equal(gi, pi) and np.array_equal(u32(gv), u32(pv))
    assert (out["dets"][0]["frame"] == 0).all()
    # and the best-class form is the fixture's (main.c:1039-1046)
    wi, wv = c["best_idx"], c["best_val"]
    bi, bv = af.best_records(rows[:n])
    assert np.array_equal(bi, wi) and np.array_equal(u32(bv), wv)
    # the default tail on the same tensor computes other numbers
    core = hipdrv.postprocess(ctx, buf.addr, 1, [c["w"]], [c["h"]], c["thresh"], c["nms"], final_q=q, cap=8192, want_rows=True, want_proc=True)
    assert (u32(core["proc"][0]) != c["proc"]).sum() > 1000
    buf.free()


@pytest.mark.parametrize("name", af.FLOAT_CASES)
def test_gpu_app_tail_float_entry_within_the_float_tolerances(ctx, name):
    """device expf instead of the host-filled tables: the same candidates, values within the tolerances the existing float entry is
    granted against the reference"""
    c = af.case(name)
    t, q = af.tensor(c["tensor"])
    fbuf = hipdrv.DevBuf(t.astype(np.float32) * np.float32(2.0 ** -q))
    n = c["total"]
    out = hipdrv.postprocess(ctx, fbuf.addr, 1, [c["w"]], [c["h"]], c["thresh"], c["nms"], cap=8192, want_rows=True, want_proc=True, tail="app")
    want_rows, want_proc = c["rows"].view(np.float32), c["proc"].view(np.float32)
    assert int(out["totals"][0]) == n
    assert np.allclose(out["proc"][0], want_proc, rtol=2e-6, atol=1e-9)
    rows = out["rows"][0]
    assert np.array_equal(rows[:n, 5:] > 0, want_rows[:, 5:] > 0), "the same candidates and kept probabilities"
    assert np.allclose(rows[:n], want_rows, rtol=1e-5, atol=1e-7) and not rows[n:].any()
    fbuf.free()


def test_gpu_app_tail_batch_from_the_network_equals_host_rows_in_order():
    model = synth.SynthModel(seed=1)
    B = 12
    frames = np.concatenate([synth.frames(7, 1), synth.frames(321, B - 1)])
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    fd = hipdrv.DevBuf(frames)
    rd = hipdrv.DevBuf(nbytes=B * 425 * 169 * 2)
    q = c.run_batch_ptr(fd.addr, B, rd.addr, 0)
    region = rd.get(np.int16, (B, 425, 13, 13))
    assert np.array_equal(region[0].reshape(-1), FULL["i16/std/region_raw_i16"])
    ws = [768, 416, 500, 640, 1, 1920, 333, 416, 100, 4000, 640, 77]
    hs = [576, 416, 375, 480, 1, 1080, 999, 415, 100, 3000, 360, 78]
    for thresh, nms in ((0.004, 0.45), (0.02, 0.3), (0.24, 0.45), (0.02, 0.0)):
        out = hipdrv.postprocess(c, rd.addr, B, ws, hs, thresh, nms, final_q=q, cap=4096, want_rows=True, tail="app")
        rows, totals = af.host_tail(region, q, ws, hs, thresh, nms, threads=8)
        assert np.array_equal(out["totals"], totals), (thresh, nms)
        if thresh < 0.01:
            assert totals.min() > 300
        assert np.array_equal(u32(out["rows"]), u32(rows)), (thresh, nms, [f for f in range(B) if not np.array_equal(u32(out["rows"][f]), u32(rows[f]))])
    fd.free(); rd.free(); c.close()


def _records_equal(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def test_gpu_images_entry_with_the_app_tail_flag():
    dog = DOG["rgb"]

    def natural(w, h):
        return np.ascontiguousarray(dog[np.arange(h) * dog.shape[0] // h][:, np.arange(w) * dog.shape[1] // w])

    yuyv = [rgb_to_yuyv(natural(768, 576)), rgb_to_yuyv(natural(320, 240)), rgb_to_yuyv(natural(300, 700))]
    rgb = [formula(f) for f in yuyv]
    c = hipdrv.Yolo2Hip(0)
    c.load_model(synth.SynthModel(seed=1, obj_bias=2.0))
    thresh, nms = 0.1, 0.45
    for imgs, fmt in ((rgb, "rgb24"), (yuyv, "yuyv")):
        region, q = c.run_images_host(imgs, 2, pixfmt=fmt)
        rd = hipdrv.DevBuf(np.ascontiguousarray(region, dtype=np.int16))
        ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
        for best in (True, False):
            got = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=4096, best_class=best, pixfmt=fmt, tail="app")
            core = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=4096, best_class=best, pixfmt=fmt)
            assert got["final_q"] == q
            if not best:
                want = hipdrv.postprocess(c, rd.addr, len(imgs), ws, hs, thresh, nms, final_q=q, cap=4096, tail="app")
                assert np.array_equal(got["counts"], want["counts"]) and got["counts"].min() > 0
                assert all(_records_equal(got["dets"][f], want["dets"][f]) for f in range(len(imgs)))
            else:
                rows = hipdrv.postprocess(c, rd.addr, len(imgs), ws, hs, thresh, nms, final_q=q, cap=1, want_rows=True, tail="app")
                for f in range(len(imgs)):
                    wi, wv = af.best_records(rows["rows"][f, :rows["totals"][f]])
                    gi, gv = af.rec_arrays(got["dets"][f])
                    assert len(wi) > 0 and np.array_equal(gi, wi) and np.array_equal(u32(gv), u32(wv)) and (got["dets"][f]["frame"] == f).all()
            assert not all(_records_equal(got["dets"][f], core["dets"][f]) for f in range(len(imgs))), "the flag is not ignored"
        rd.free()
    c.close()


@pytest.mark.parametrize("precision", ["fp16", "fp32fast"])
def test_gpu_images_f16_and_multi_entries_honour_the_flag(precision):
    """the _dets_f16 entries and the multi-device entries with YOLO2_DETS_APP_TAIL: the float app tail on the region tensor the same
    pass returns to the host, and the single context's records from two shards"""
    rgb = DOG["rgb"]
    imgs = [rgb, rgb[::2, ::2].copy(), rgb[100:400, 50:700].copy()]
    ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
    thresh, nms = 0.05, 0.45
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    c = hipdrv.Yolo2Hip(0)
    c.load_weights_fp32(model.weights_f32(), model.bias_f32())
    region = c.run_images_f16_host(imgs, 2, split=precision == "fp32fast")
    buf = hipdrv.DevBuf(np.ascontiguousarray(region))
    want = hipdrv.postprocess(c, buf.addr, len(imgs), ws, hs, thresh, nms, cap=4096, tail="app")
    buf.free()
    got = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=4096, best_class=False, precision=precision, tail="app")
    core = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=4096, best_class=False, precision=precision)
    best = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=845, precision=precision, tail="app")
    c.close()
    assert np.array_equal(got["counts"], want["counts"]) and want["counts"].min() > 5
    assert all(_records_equal(got["dets"][f], want["dets"][f]) for f in range(len(imgs)))
    assert not all(_records_equal(got["dets"][f], core["dets"][f]) for f in range(len(imgs))), "the flag is not ignored"
    m = hipdrv.Yolo2HipMulti([0, 0])
    m.load_model_fp32(model)
    gm = hipdrv.run_images_dets(m._m, imgs, 2, thresh, nms, cap=845, multi=True, precision=precision, tail="app")
    m.close()
    assert np.array_equal(gm["counts"], best["counts"]) and all(_records_equal(gm["dets"][f], best["dets"][f]) for f in range(len(imgs)))
    if precision == "fp16":      # the int16 multi entry once
        m = hipdrv.Yolo2HipMulti([0, 0])
        m.load_model(model)
        gi = hipdrv.run_images_dets(m._m, imgs, 2, thresh, nms, cap=845, multi=True, tail="app")
        m.close()
        c = hipdrv.Yolo2Hip(0)
        c.load_model(model)
        si = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=845, tail="app")
        sc = hipdrv.run_images_dets(c._h, imgs, 2, thresh, nms, cap=845)
        c.close()
        assert all(_records_equal(gi["dets"][f], si["dets"][f]) for f in range(len(imgs)))
        assert not all(_records_equal(si["dets"][f], sc["dets"][f]) for f in range(len(imgs)))


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def _print_block(recs_idx, recs_val, thresh, names):
    """yolo2_print_detections (linux_app/src/yolo2_postprocess.c:303-341) on best-class records"""
    bar = "=" * 40
    lines = ["", bar, "Detections (thresh=%.2f):" % thresh, bar]
    printed = 0
    for (_, cls), (p, x, y, w, h) in zip(recs_idx, recs_val):
        if p > np.float32(thresh):
            name = names[cls] if cls < len(names) else "unknown"
            lines.append("  %-16s prob=%.2f%% box=[x=%.3f y=%.3f w=%.3f h=%.3f]" % (name, float(np.float32(p) * np.float32(100.0)), x, y, w, h))
            printed += 1
    lines += ["  No detections above threshold"] if printed == 0 else ["", "Total: %d detections" % printed]
    return "\n".join(lines + [bar, "", ""])


def test_reference_app_is_the_judge(ctx, tmp_path):
    """the reference's own application, linked against the library, in image mode: the activated tensor it dumps and the detection
    block it prints are what the app tail makes of the same region tensor"""
    if not os.path.exists(APP):
        pytest.skip("oracle/_ref/yolo2_linux is built in the build container only (make -C oracle ref_app)")
    mg = _mg()
    model = synth.SynthModel(seed=1, **mg.Q_SETS["std"])
    wdir = tmp_path / "weights"
    model.write_files(str(wdir), fp32=False, int16=True)
    img = tmp_path / "frame416.ppm"
    rgb = mg.refapp_image()
    with open(img, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())
    names_path = os.path.join(PKG, "config", "coco.names")
    cmd = [APP, "-i", str(img), "-w", str(wdir), "-c", os.path.join(PKG, "config", "yolov2.cfg"), "-l", names_path, "-t", "0.05", "-v", "1"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, YOLO2_VERBOSE="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    proc = np.loadtxt(str(tmp_path / "yolov2_region_proc_hw.txt"), dtype=np.float64).astype(np.float32)     # %.9g round-trips a float32
    assert proc.size == af.ELEMS
    q = int(REFAPP["std/final_q"])
    buf = hipdrv.DevBuf(REFAPP["std/region_raw_i16"].astype(np.int16))
    thresh = float(np.float32(0.05))
    out = hipdrv.postprocess(ctx, buf.addr, 1, [416], [416], thresh, float(np.float32(0.45)), final_q=q, cap=1, want_rows=True, want_proc=True, tail="app")
    buf.free()
    assert np.array_equal(u32(out["proc"][0]), u32(proc)), f"{int((u32(out['proc'][0]) != u32(proc)).sum())} of {proc.size} activated values differ"
    n = int(out["totals"][0])
    if n == 0:
        assert "\nNo detections found above threshold 0.05\n" in r.stdout
        return
    names = [s.strip() for s in open(names_path) if s.strip()]
    bi, bv = af.best_records(out["rows"][0, :n])
    want = _print_block(bi, bv, thresh, names)
    m = re.search(r"\n={40}\nDetections \(thresh=.*?\n={40}\n.*?\n={40}\n\n", r.stdout, re.S)
    assert m, r.stdout[-3000:]
    assert m.group(0) == want, (m.group(0)[:2000], want[:2000])


def test_gpu_app_tail_rate(ctx):
    """both tails on the batch-256 tensor of test_gpu_postprocess_dog_and_throughput, in one process: the app tail must reach the
    floor the project sets for the tail (profiles/r11_app_tail.txt records a run)"""
    q = int(DOG["i16/final_q"])
    B = 256
    rng = np.random.default_rng(0)
    base = DOG["i16/region_raw_i16"].astype(np.int32)
    batch = np.stack([np.clip(np.roll(base, 173 * f) + rng.integers(-2, 3, base.size), -32768, 32767) for f in range(B)]).astype(np.int16)
    rd = hipdrv.DevBuf(batch)
    ws, hs = [768] * B, [576] * B
    fps = {}
    for tail in ("core", "app"):
        hipdrv.postprocess(ctx, rd.addr, B, ws, hs, 0.24, 0.45, final_q=q, cap=128, tail=tail)
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            hipdrv.postprocess(ctx, rd.addr, B, ws, hs, 0.24, 0.45, final_q=q, cap=128, tail=tail)
        fps[tail] = B / ((time.perf_counter() - t0) / reps)
    print(f"GPU region+boxes+NMS at batch {B} (thresh 0.24, nms 0.45): core tail {fps['core']:.0f} frames/s, app tail {fps['app']:.0f} frames/s")
    rows, totals = af.host_tail(batch[:8], q, ws[:8], hs[:8], 0.24, 0.45, threads=8)
    got = hipdrv.postprocess(ctx, rd.addr, 8, ws[:8], hs[:8], 0.24, 0.45, final_q=q, cap=128, want_rows=True, tail="app")
    assert np.array_equal(got["totals"], totals) and np.array_equal(u32(got["rows"]), u32(rows))
    rd.free()
    assert fps["app"] >= 30000, fps


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    return subprocess.run([os.path.join(PKG, "yolov2_detect"), "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names",
                           os.path.join(PKG, "config", "coco.names")] + args, capture_output=True, text=True, cwd=str(cwd),
                          env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_tail_app_streams_the_app_tails_records(tmp_path):
    """--tail app on a raw RGB24 stream: --post gpu and --post host write the same JSONL, its numbers are those of
    run_images_dets(tail="app") in the reference's %.6f, they differ from --tail core's, and an unknown value is a usage error"""
    w, h = 320, 240
    dog = DOG["rgb"]
    base = np.ascontiguousarray(dog[np.arange(h) * dog.shape[0] // h][:, np.arange(w) * dog.shape[1] // w])
    frames = [np.ascontiguousarray(np.roll(base, 14 * k, axis=1)) for k in range(4)]
    (tmp_path / "video.rgb").write_bytes(b"".join(f.tobytes() for f in frames))
    model = synth.SynthModel(seed=1, obj_bias=2.0)
    model.write_files(str(tmp_path / "weights"), fp32=False, int16=True)
    common = ["--weights", str(tmp_path / "weights"), "--batch", "3", "--thresh", "0.1", "--chunk-batches", "1", "--precision", "int16",
              "--video-raw", str(tmp_path / "video.rgb"), "--video-pix-fmt", "rgb24", "--video-width", str(w), "--video-height", str(h)]
    out = {}
    for tag, extra in (("app_gpu", ["--tail", "app"]), ("app_host", ["--tail", "app", "--post", "host"]), ("core_gpu", ["--tail", "core"]), ("default", [])):
        path = tmp_path / f"{tag}.jsonl"
        r = _cli(common + extra + ["--jsonl", str(path)], tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[tag] = [json.loads(line) for line in path.read_text().splitlines()]
        assert len(out[tag]) == len(frames)
    assert out["app_gpu"] == out["app_host"] and out["core_gpu"] == out["default"]
    assert out["app_gpu"] != out["core_gpu"]
    c = hipdrv.Yolo2Hip(0)
    c.load_model(model)
    want = hipdrv.run_images_dets(c._h, frames, 3, 0.1, 0.45, tail="app")
    c.close()
    n = 0
    for f, line in enumerate(out["app_gpu"]):
        recs = [r for r in want["dets"][f] if r["prob"] > np.float32(0.1)]
        assert len(recs) == len(line["detections"])
        for r, d in zip(recs, line["detections"]):
            assert d["class_id"] == int(r["cls"]) and "%.6f" % d["prob"] == "%.6f" % r["prob"]
            assert ["%.6f" % d["bbox_norm"][k] for k in "xywh"] == ["%.6f" % r[k] for k in "xywh"]
            n += 1
    assert n > 4
    r = _cli(common + ["--tail", "bogus"], tmp_path)
    assert r.returncode != 0 and "--tail" in r.stderr
