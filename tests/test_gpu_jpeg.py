"""GPU tests of the annotated frame as JPEG: yolo2_hip_jpeg_encode_rgb24, yolo2_hip_annotate_images_pix_jpeg_host, its multi form
and the CLI's --annotated-format jpg write exactly the bytes the reference's MJPEG streamer sends.  The expected side is the fixture
the compiled reference made (tests/golden/jpeg.npz) and, at the sizes it does not hold, the host restatement y2h_write_jpg_rgb24
behind the host painter y2h_draw_detections_rgb24, which tests/test_jpeg_host.py and tests/test_draw_host.py pin to their fixtures -
never the code under test."""
import os
import subprocess

import numpy as np
import pytest

import orclib
from drawref import case as draw_case, host_draw, records
from jpegref import CASES, case, host_jpg
from yolo2_amd import hipdrv, synth
from yuyvref import formula

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
PKG = os.path.join(ROOT, "yolo-fpga-accelerator_amd")
CLI = os.path.join(PKG, "yolov2_detect")
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))["rgb"]          # 768 x 576
NAMES = [s.strip() for s in open(os.path.join(PKG, "config", "coco.names")) if s.strip()]
C = hipdrv.C


@pytest.mark.parametrize("name", CASES)
def test_jpeg_encode_equals_the_reference(name):
    rgb, quality, want = case(name)
    got = hipdrv.jpeg_encode(rgb, quality)
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("quality", [1, 50, 80, 100])
@pytest.mark.parametrize("w,h", [(7, 9), (9, 8), (17, 33), (320, 240)])
def test_jpeg_encode_equals_the_restatement_at_other_sizes(w, h, quality):
    """320x240 is 1200 MCUs = 3600 blocks: 29 workgroups of kJpegBlocks = 128 blocks in stages A - C, the last with 16 blocks.
    Noise at quality 100 gives an unstuffed scan of several hundred kB: more than 64 segments of kJpegSegBytes = 4096 bytes, so the
    workgroups of stage D (at most 64 per frame) loop, and the last segment is partial."""
    rng = np.random.default_rng(w * 1000 + h)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = host_jpg(rgb, quality)
    if (w, h, quality) == (320, 240, 100):
        assert len(want) - 609 > 64 * 4096
    got = hipdrv.jpeg_encode(rgb, quality)
    assert len(got) == len(want) and got == want


def test_a_natural_frame_across_many_workgroups_and_segments():
    """the 768x576 dog frame: 6912 MCUs = 20736 blocks = 162 workgroups of 128 blocks, about 25 segments of 4096 unstuffed bytes;
    a 763x571 cut of it has ragged edges: 96 x 72 MCUs still, with repeated edge pixels"""
    for rgb in (DOG, np.ascontiguousarray(DOG[3:574, 2:765])):
        want = host_jpg(rgb, 80)
        got = hipdrv.jpeg_encode(rgb, 80)
        assert len(got) == len(want) and got == want


def test_frames_whose_per_frame_scans_take_several_rounds():
    """k_jpeg_scan_groups and k_jpeg_scan_segs scan kJpegScan = 256 entries per round and carry a running total into the next.
    1283x725 is 161 x 91 MCUs = 43,953 blocks = 344 groups of kJpegBlocks = 128 blocks (the last with 49): two rounds of the group
    scan, with ragged edges both ways; its content is the dog frame continued by wrapping, with a band of noise.  640x480 noise at
    quality 100 has an unstuffed scan above 1 MB = more than 256 segments of kJpegSegBytes = 4096 bytes: two rounds of the segment
    scan (and 113 groups, and every one of stage D's at most 64 workgroups loops several times)."""
    big = np.ascontiguousarray(np.pad(DOG, ((0, 725 - 576), (0, 1283 - 768), (0, 0)), mode="wrap"))
    big[300:420] = np.random.default_rng(7).integers(0, 256, (120, 1283, 3), dtype=np.uint8)
    want = host_jpg(big, 80)
    got = hipdrv.jpeg_encode(big, 80)
    assert len(got) == len(want) and got == want
    noise = np.random.default_rng(8).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    want = host_jpg(noise, 100)
    stuffed = want[607:-2].count(b"\xff\x00")
    assert len(want) - 609 - stuffed > 256 * 4096
    got = hipdrv.jpeg_encode(noise, 100)
    assert len(got) == len(want) and got == want


def test_odd_addresses_a_small_capacity_and_guard_bytes():
    L = hipdrv.lib()
    rgb, quality, want = case("rand_64x48_q80")
    n = len(want)
    src = hipdrv.DevBuf(np.concatenate([np.zeros(3, dtype=np.uint8), rgb.reshape(-1)]))
    size = C.c_size_t(0)
    for shift, cap in ((1, n), (3, n + 40), (5, n - 1), (7, 700), (2, 607), (1, 1)):
        dst = hipdrv.DevBuf(np.full(n + 128, 0xA5, dtype=np.uint8))
        rc = L.yolo2_hip_jpeg_encode_rgb24(src.addr + 3, 64, 48, quality, dst.addr + shift, cap, C.byref(size), None)
        out = dst.get(np.uint8, (n + 128,))
        dst.free()
        assert size.value == n, (shift, cap)
        if cap >= n:
            assert rc == 0, hipdrv.lib().yolo2_hip_last_error()
        else:
            assert rc == hipdrv.YOLO2_ERROR and b"too small" in L.yolo2_hip_last_error()
        k = min(cap, n)
        assert out[shift:shift + k].tobytes() == want[:k], (shift, cap)
        assert (out[:shift] == 0xA5).all() and (out[shift + k:] == 0xA5).all(), (shift, cap)
    # capacity 0 needs no output address
    assert L.yolo2_hip_jpeg_encode_rgb24(src.addr + 3, 64, 48, quality, 0, 0, C.byref(size), None) == hipdrv.YOLO2_ERROR and size.value == n
    src.free()


def test_bad_arguments_are_refused():
    L = hipdrv.lib()
    buf = hipdrv.DevBuf(nbytes=4096)
    size = C.c_size_t(0)
    for w, h in ((0, 4), (4, 0), (-2, 4), (65536, 1), (1, 65536)):
        assert L.yolo2_hip_jpeg_encode_rgb24(buf.addr, w, h, 80, buf.addr, 4096, C.byref(size), None) == hipdrv.YOLO2_ERROR
        assert b"1..65535" in L.yolo2_hip_last_error()
        assert hipdrv.jpeg_bound(w, h) == 0
    assert L.yolo2_hip_jpeg_encode_rgb24(0, 4, 4, 80, buf.addr, 4096, C.byref(size), None) == hipdrv.YOLO2_ERROR
    assert L.yolo2_hip_jpeg_encode_rgb24(buf.addr, 4, 4, 80, 0, 4096, C.byref(size), None) == hipdrv.YOLO2_ERROR
    assert L.yolo2_hip_jpeg_encode_rgb24(buf.addr, 65535, 65535, 80, buf.addr, 4096, C.byref(size), None) == hipdrv.YOLO2_ERROR
    assert b"too large" in L.yolo2_hip_last_error()
    assert hipdrv.jpeg_bound(65535, 65535) == 0 and hipdrv.jpeg_bound(12000, 10000) == 0      # no bound for a size the entries refuse
    buf.free()
    assert hipdrv.jpeg_bound(8, 8) == 607 + 2 * ((3 * 1660 + 7) // 8) + 2
    assert all(hipdrv.jpeg_bound(case(n)[0].shape[1], case(n)[0].shape[0]) >= len(case(n)[2]) for n in CASES)


def _random_records(rng, n, frame=0):
    """n records all over (and partly off) the frame, every class, probabilities on both sides of 0.24"""
    box = np.stack([rng.uniform(.05, 1., n), rng.uniform(-.1, 1.1, n), rng.uniform(-.1, 1.1, n), rng.uniform(0, .5, n), rng.uniform(0, .5, n)], axis=1)
    return records(rng.integers(0, 80, n), box.astype(np.float32), frame)


def _mixed_set():
    """nine RGB frames from 1x1 to 320x240 with their records [9][845] and counts (the construction of tests/test_gpu_draw.py): the
    draw fixture's 845-record frame, a frame with 300 records all over it, zero-record frames, a count above the capacity"""
    rng = np.random.default_rng(9)
    sizes = [(1, 1), (64, 48), (320, 240), (33, 17), (2, 2), (160, 120), (97, 3), (5, 211), (128, 96)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    many = draw_case("many845")
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


@pytest.fixture(scope="module")
def mixed():
    frames, dets, counts = _mixed_set()
    painted = [host_draw(frames[f], dets[f, :min(counts[f], 845)], .24, NAMES) for f in range(9)]
    want = [host_jpg(p[0], 80) for p in painted]
    return frames, dets, counts, painted, want


def test_batched_entry_equals_the_host_painter_and_the_restatement(mixed):
    frames, dets, counts, painted, want = mixed
    assert painted[1][1] == 845 and painted[5][1] == 0 and painted[2][1] > 128
    ctx = hipdrv.Yolo2Hip(0)      # no weights
    for batch in (4, 2, 64):      # nine frames at batch 4: three chunks, a ragged last one, sizes that differ inside a chunk
        outs, drawn = ctx.annotate_images(frames, dets, counts, batch, .24, labels=NAMES, jpeg_quality=80)
        for f in range(9):
            assert drawn[f] == painted[f][1], (batch, f)
            assert isinstance(outs[f], bytes) and len(outs[f]) == len(want[f]) and outs[f] == want[f], (batch, f)
    # a frame without records in RGB24 is a pure encode
    assert want[5] == host_jpg(frames[5], 80)
    # from YUYV, labels = NULL, another quality
    rng = np.random.default_rng(10)
    yuyv = [rng.integers(0, 256, (fr.shape[0], fr.shape[1] + (fr.shape[1] & 1), 2), dtype=np.uint8) for fr in frames]
    outs, drawn = ctx.annotate_images(yuyv, dets, counts, 4, .24, pixfmt="yuyv", jpeg_quality=55)
    for f in range(9):
        img, n = host_draw(formula(yuyv[f]), dets[f, :min(counts[f], 845)], .24, None)
        assert drawn[f] == n and outs[f] == host_jpg(img, 55), f
    ctx.close()


def test_batched_entry_with_one_capacity_too_small(mixed):
    frames, dets, counts, painted, want = mixed
    ctx = hipdrv.Yolo2Hip(0)
    L = hipdrv.lib()
    for short, cap in ((2, len(want[2]) - 1), (5, 1000), (0, 0), (8, 607)):
        caps = [len(w) + 9 for w in want]
        caps[short] = cap
        rc, outs, sizes, drawn = hipdrv.annotate_images_jpeg_raw(ctx._h, frames, dets, counts, 4, .24, 80, caps, labels=NAMES, guard=16)
        assert rc == hipdrv.YOLO2_ERROR and b"too small for frame %d" % short in L.yolo2_hip_last_error(), short
        for f in range(9):
            k = min(caps[f], len(want[f]))
            assert int(sizes[f]) == len(want[f]), (short, f)
            assert outs[f][:k].tobytes() == want[f][:k], (short, f)
            assert (outs[f][k:] == 0xA5).all(), (short, f)
    # exact capacities are enough
    rc, outs, sizes, drawn = hipdrv.annotate_images_jpeg_raw(ctx._h, frames, dets, counts, 3, .24, 80, [len(w) for w in want], labels=NAMES, guard=16)
    assert rc == 0 and all(outs[f][:len(want[f])].tobytes() == want[f] and (outs[f][len(want[f]):] == 0xA5).all() for f in range(9))
    ctx.close()


def test_multi_entry_equals_the_restatement(mixed):
    frames, dets, counts, painted, want = mixed
    m = hipdrv.Yolo2HipMulti([0, 0])
    outs, drawn = m.annotate_images(frames, dets, counts, 2, .24, labels=NAMES, jpeg_quality=80)
    m.close()
    assert [int(d) for d in drawn] == [p[1] for p in painted]
    for f in range(9):
        assert outs[f] == want[f], f


def test_refusals_launch_nothing_and_memory_balances(mixed):
    frames, dets, counts, painted, want = mixed
    L = hipdrv.lib()
    base = hipdrv.live_bytes()
    ctx = hipdrv.Yolo2Hip(0)
    held = hipdrv.live_bytes()
    caps = [len(w) for w in want]
    # the encoder's own refusals come before anything is allocated: a null capacity list (through the raw call), a bad size
    n, ptrs, ws, hs, fmt, keep = hipdrv._image_args(frames, "rgb24")
    outs = [np.full(c + 1, 0xA5, dtype=np.uint8) for c in caps]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    sizes = np.zeros(n, dtype=np.uint64)
    cap_arr = np.array(caps, dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    for kw in (dict(caps=None), dict(sizes=None), dict(outs=None)):
        rc = L.yolo2_hip_annotate_images_pix_jpeg_host(ctx._h, ptrs, ws, hs, fmt, n, 4, vp(dets), 845, vp(cnt), .24, None, 0, 80,
                                                       kw.get("outs", optrs), kw.get("caps", vp(cap_arr)), kw.get("sizes", vp(sizes)), None)
        assert rc == hipdrv.YOLO2_ERROR and b"null" in L.yolo2_hip_last_error(), kw
        assert hipdrv.live_bytes() == held
    assert all((o == 0xA5).all() for o in outs)
    got, drawn = ctx.annotate_images(frames, dets, counts, 4, .24, labels=NAMES, jpeg_quality=80)
    assert got == want
    assert hipdrv.live_bytes() != held
    ctx.close()
    assert hipdrv.live_bytes() == base


# ------------------------------------------------------------------ CLI

def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def test_cli_writes_the_entrys_streams(tmp_path):
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
    ctx.close()
    res = _cli(common + ["--annotate-gpu", "--save-annotated-dir", str(tmp_path / "q80"), "--annotated-format", "jpg"], tmp_path)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    res = _cli(common + ["--annotate-gpu", "--save-annotated-dir", str(tmp_path / "q35"), "--annotated-format", "jpg", "--jpeg-quality", "35"], tmp_path)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    drawn = 0
    for f, im in enumerate(images):
        painted, n = host_draw(im, r["dets"][f], .1, NAMES)
        drawn += n
        assert (tmp_path / "q80" / f"frame_{f + 1:06d}.jpg").read_bytes() == host_jpg(painted, 80), f
        assert (tmp_path / "q35" / f"frame_{f + 1:06d}.jpg").read_bytes() == host_jpg(painted, 35), f
        assert not (tmp_path / "q80" / f"frame_{f + 1:06d}.ppm").exists()
    assert drawn > 4
    res = _cli(common + ["--save-annotated-dir", str(tmp_path / "x"), "--annotated-format", "jpg"], tmp_path)
    assert res.returncode != 0 and "--annotated-format jpg encodes the frames of --annotate-gpu" in res.stdout + res.stderr
