"""The int8 pass from image bytes on the GPU (run with -m gpu): yolo2_hip_run_images_pix_int8_host / _dets_int8 and the kernel in
front of them, k_i8_front_pix (letterbox + input rule + layer 0 in one k step + 2x2 pool).  Every check is equality: the int32 sum
is exact, so the fused front may differ from tests/i8ref.py and from the frames route in no bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import apptail_fix as af
import i8ref
import orclib
from yolo2_amd import hipdrv, net, synth

pytestmark = pytest.mark.gpu

FUSED = {"rgb24": "k_i8_front_u8", "grey8": "k_i8_front_u8", "yuyv": "k_i8_front_yuyv"}
UNFUSED = {"rgb24": "k_letterbox_u8_batch", "grey8": "k_letterbox_u8_batch", "yuyv": "k_letterbox_yuyv_batch"}


def _images():
    rng = np.random.default_rng(2026)
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    rgb = [u8(416, 416, 3),      # no resize, no bands
           u8(480, 640, 3),      # bands above and below: canvas edge rows are 0.5 next to the conv's zero padding
           u8(500, 300, 3),      # bands left and right
           u8(1, 1, 3), u8(5, 7, 3),
           u8(1080, 1920, 3),    # large downscale
           u8(77, 333, 3)]       # the fitted region's edges fall inside tiles
    return {"rgb24": rgb, "grey8": [u8(45, 123)], "yuyv": [u8(576, 768, 2), u8(18, 34, 2)]}


IMGS = _images()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_u32(a), _u32(b))


def _host_frame(im, fmt):
    """the host letterbox of one image: float32 [3][416][416]"""
    if fmt == "yuyv":
        h, w = im.shape[:2]
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        lib = orclib.host()
        lib.y2h_yuyv_to_rgb24.argtypes = [hipdrv.C.c_void_p, hipdrv.C.c_void_p, hipdrv.C.c_int, hipdrv.C.c_int]
        assert lib.y2h_yuyv_to_rgb24(im.ctypes.data, rgb.ctypes.data, w, h) == 0
        im = rgb
    if im.ndim == 2:
        im = np.repeat(im[:, :, None], 3, axis=2)
    chw = np.ascontiguousarray(im.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    out = np.zeros((3, 416, 416), dtype=np.float32)
    orclib.host().y2h_letterbox(chw, im.shape[1], im.shape[0], 3, 416, 416, out)
    return out


class Net:
    pass


@pytest.fixture(scope="module")
def netw():
    """SynthModel(seed=1) calibrated as tests/test_gpu_i8.py does; per pixel format the region tensors of the frames route on the
    library's own letterboxed frames.  Computed once, shared, left unchanged."""
    n = Net()
    n.model = synth.SynthModel(seed=1)
    n.ctx = hipdrv.Yolo2Hip(0)
    n.ctx.load_weights_fp32(n.model.weights_f32(), n.model.bias_f32())
    n.cal = n.ctx.calibrate_int8(frames=synth.frames(40, 4), batch=4)
    n.ctx.load_model(n.cal)
    n.want = {}
    for fmt, imgs in IMGS.items():
        frames = np.stack([hipdrv.letterbox_pix(im, fmt) for im in imgs])
        n.want[fmt] = n.ctx.run_batch_int8_host(frames)
    yield n
    n.ctx.close()


def _layer0(cal):
    w8 = cal.w8[:32 * 27].reshape(32, 3, 3, 3)
    return w8, cal.bias32[:32], cal.weight_q[:32]


# ------------------------------------------------------------------ 1. the front against numpy

@pytest.mark.parametrize("fmt,k", [(fmt, k) for fmt in IMGS for k in range(len(IMGS[fmt]))])
def test_front_kernel_equals_numpy_on_the_host_letterbox(netw, fmt, k):
    im = IMGS[fmt][k]
    w8, b32, qw = _layer0(netw.cal)
    aq = netw.cal.act_q
    x = i8ref.quantize_input(_host_frame(im, fmt)[None], aq[0])
    want = i8ref.pool(i8ref.conv(x, w8, b32, qw, int(aq[0]), int(aq[1]), True))[0].astype(np.int8)
    assert want.min() < 0 < want.max()
    if fmt == "rgb24" and im.shape[:2] == (480, 640):
        # 640x480 fits as 416x312 at canvas rows 52..363: pooled rows 1..24 see the band only (conv rows 2..49, taps up to row 50),
        # pooled row 25 (conv rows 50 and 51) reaches image row 52; pooled row 0 touches the conv's zero padding, which is not 0.5
        assert np.array_equal(want[:, 1], want[:, 2]) and np.array_equal(want[:, 23], want[:, 24])
        assert not np.array_equal(want[:, 24], want[:, 25]) and not np.array_equal(want[:, 0], want[:, 1])
    netw.ctx.run_images_int8_host([im], 1, pixfmt=fmt)
    assert netw.ctx.images_front_kernel_int8() == FUSED[fmt]
    got, q = netw.ctx.debug_i8_tensor(1, 0)
    assert q == aq[1] and got.shape == (32, 208, 208)
    same = got == want
    assert same.all(), f"{int((~same).sum())} of {same.size} differ, first at {tuple(np.argwhere(~same)[0])}"


# ------------------------------------------------------------------ 2. fragment map, k map and pool window with one-hot weights

def test_one_hot_weights_pin_the_k_map_and_the_pool_window(netw):
    cal = netw.cal
    w8, b32, wq, aq = cal.w8.copy(), cal.bias32.copy(), cal.weight_q.copy(), cal.act_q.copy()
    w0 = np.zeros((32, 3, 9), dtype=np.int8)
    for m in range(27):
        w0[m, m % 3, m // 3] = 1
    w8[:32 * 27] = w0.reshape(-1)
    b32[:32] = 0
    b32[27:32] = [-1000, -1, 0, 1, 1000]
    wq[:32] = 0
    delta = int(aq[0]) - int(aq[1])
    aq[1] = aq[0]                                                 # s of layer 0 = 0
    wq[32:96] = np.clip(wq[32:96] - delta, -8, 24)                # layer 2 keeps its shift where the Q range allows (only layer 1 is read)
    rng = np.random.default_rng(7)
    im = rng.integers(0, 256, (416, 416, 3), dtype=np.uint8)
    x = i8ref.quantize_input(_host_frame(im, "rgb24"), aq[0]).astype(np.int64)      # [3][416][416]
    assert x.min() >= 0 and x.max() > 32 and not np.array_equal(x[0], x[1]) and not np.array_equal(x[0], x[0].T)
    ctx = hipdrv.Yolo2Hip(0)
    try:
        ctx.load_weights_int8(w8, b32, wq, aq)
        ctx.run_images_int8_host([im], 1)
        assert ctx.images_front_kernel_int8() == "k_i8_front_u8"
        got, q = ctx.debug_i8_tensor(1, 0)
    finally:
        ctx.close()
    assert q == aq[0]
    for m in range(27):
        c, ky, kx = m % 3, (m // 3) // 3, (m // 3) % 3
        pad = np.zeros((418, 418), dtype=np.int64)
        pad[1:417, 1:417] = x[c]
        conv = pad[ky:ky + 416, kx:kx + 416]                      # out(y, x) = in(y + ky - 1, x + kx - 1), zeros beyond the canvas
        want = conv.reshape(208, 2, 208, 2).max(axis=(1, 3))
        assert np.array_equal(got[m], want), f"channel {m} (c {c}, tap {ky},{kx})"
    for m, v in zip(range(27, 32), (-100, 0, 0, 1, 127)):
        assert (got[m] == v).all(), (m, v, np.unique(got[m]))


# ------------------------------------------------------------------ 3. the whole route

@pytest.mark.parametrize("fmt", list(IMGS))
def test_images_route_equals_the_frames_route_and_the_unfused_route(netw, fmt):
    imgs = IMGS[fmt]
    got = netw.ctx.run_images_int8_host(imgs, len(imgs), pixfmt=fmt)
    assert netw.ctx.images_front_kernel_int8() == FUSED[fmt]
    assert _same_bits(got, netw.want[fmt])
    assert np.isfinite(got).all() and got.std() > 0.1
    netw.ctx.set_option("i8_no_front", 1)
    try:
        ref = netw.ctx.run_images_int8_host(imgs, len(imgs), pixfmt=fmt)
        name = netw.ctx.images_front_kernel_int8()
        x8, q = netw.ctx.debug_i8_tensor(-1, 0)                    # the frames route ran: its quantised input exists
        assert q == netw.cal.act_q[0] and x8.shape == (3, 416, 416) and netw.ctx.debug_i8_tensor(0, 0)[0].shape == (32, 416, 416)
    finally:
        netw.ctx.set_option("i8_no_front", None)
    assert name.split(" + ") == [UNFUSED[fmt], "k_i8_quant_input", "k_conv_i8"]
    assert _same_bits(ref, netw.want[fmt])


# ------------------------------------------------------------------ 4. chunking

def test_chunks_reuse_buffer_sets_and_a_ragged_last_chunk(netw):
    imgs = IMGS["rgb24"][:5]
    want = netw.want["rgb24"][:5]
    assert _same_bits(netw.ctx.run_images_int8_host(imgs, 2), want)              # three chunks: set 0 twice, the last one ragged
    assert _same_bits(netw.ctx.run_images_int8_host(imgs, 5), want)
    assert _same_bits(netw.ctx.run_images_int8_host(imgs, 7), want)              # batch > n
    for f in range(5):
        assert _same_bits(netw.ctx.run_images_int8_host(imgs[f:f + 1], 1), want[f:f + 1]), f


# ------------------------------------------------------------------ 5. records

ALL = 845 * 80          # every class of every box: no record list below is truncated


def _records_equal(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("tail", ["core", "app"])
def test_records_equal_the_float_tail_on_the_region_tensor(netw, tail):
    nms = 0.45
    for fmt in ("rgb24", "yuyv"):
        imgs = IMGS[fmt]
        ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
        buf = hipdrv.DevBuf(np.ascontiguousarray(netw.want[fmt]))
        try:
            thresh = 0.005
            want = hipdrv.postprocess(netw.ctx, buf.addr, len(imgs), ws, hs, thresh, nms, cap=ALL, want_rows=True, tail=tail)
            while want["counts"].max() == 0 and thresh > 1e-6:    # (chosen on the frames route's tensor, never on the fused one)
                thresh /= 4
                want = hipdrv.postprocess(netw.ctx, buf.addr, len(imgs), ws, hs, thresh, nms, cap=ALL, want_rows=True, tail=tail)
        finally:
            buf.free()
        assert want["counts"].max() > 0
        got = hipdrv.run_images_dets(netw.ctx._h, imgs, 3, thresh, nms, cap=ALL, best_class=False, precision="int8", pixfmt=fmt, tail=tail)
        assert got["final_q"] is None and np.array_equal(got["counts"], want["counts"])
        for f in range(len(imgs)):
            assert _records_equal(got["dets"][f], want["dets"][f]), (fmt, f)
            assert (got["dets"][f]["frame"] == f).all()
        best = hipdrv.run_images_dets(netw.ctx._h, imgs, 3, thresh, nms, cap=845, best_class=True, precision="int8", pixfmt=fmt, tail=tail)
        for f in range(len(imgs)):
            if tail == "core":
                recs = want["dets"][f]
                exp = np.array([rows[np.argmax(rows["prob"])] for rows in (recs[recs["det"] == d] for d in np.unique(recs["det"]))], dtype=recs.dtype)
                assert _records_equal(best["dets"][f], exp), (fmt, f)
            else:
                wi, wv = af.best_records(want["rows"][f, :want["totals"][f]])
                gi, gv = af.rec_arrays(best["dets"][f])
                assert np.array_equal(gi, wi) and np.array_equal(_u32(gv), _u32(wv)), (fmt, f)
            assert (best["dets"][f]["frame"] == f).all()


# ------------------------------------------------------------------ 6. parity hook

def test_parity_hook_after_an_images_call_and_after_a_frames_run(netw):
    imgs = IMGS["rgb24"][:3]
    netw.ctx.run_images_int8_host(imgs, 2)                         # the last chunk holds image 2 (twice: the chunk is ragged)
    frame = hipdrv.letterbox_pix(imgs[2], "rgb24")
    w, b = i8ref.model_f32(netw.model)
    ref = i8ref.ModelI8(w, b, netw.cal.act_q)
    _, layers = i8ref.forward(frame[None], ref, keep=True)
    for i in range(1, 30):
        if net.LAYERS[i].type == net.ROUTE and i != 28:
            continue
        got, q = netw.ctx.debug_i8_tensor(i, 0)
        assert np.array_equal(got, layers[i][0]), f"layer {i}"
    assert np.array_equal(netw.ctx.debug_i8_tensor(1, 1)[0], netw.ctx.debug_i8_tensor(1, 0)[0])
    for i in (-1, 0):
        with pytest.raises(hipdrv.Yolo2HipError, match="fused"):
            netw.ctx.debug_i8_tensor(i, 0)
    with pytest.raises(hipdrv.Yolo2HipError):
        netw.ctx.debug_i8_tensor(1, 2)
    netw.ctx.run_batch_int8_host(np.stack([frame, frame]))
    for i in (-1, 0):
        got, q = netw.ctx.debug_i8_tensor(i, 1)
        assert np.array_equal(got, layers[i][0]), f"layer {i}"


# ------------------------------------------------------------------ 7. refusals

def test_refusals_come_before_any_launch_and_leave_the_context_alone(netw):
    fresh = hipdrv.Yolo2Hip(0)
    try:
        with pytest.raises(hipdrv.Yolo2HipError, match="int8 weights not loaded"):
            fresh.run_images_int8_host(IMGS["rgb24"][:1], 1)
        assert fresh.images_front_kernel_int8() == ""
    finally:
        fresh.close()
    L, h = hipdrv.lib(), netw.ctx._h
    region = np.zeros((2, 425, 13, 13), dtype=np.float32)
    rp = region.ctypes.data_as(hipdrv.C.c_void_p)
    imgs = IMGS["rgb24"][3:5]

    def again():
        return _same_bits(netw.ctx.run_images_int8_host(imgs, 2), netw.want["rgb24"][3:5])

    with pytest.raises(hipdrv.Yolo2HipError, match="even width"):
        netw.ctx.run_images_int8_host([np.zeros((4, 5, 2), np.uint8)], 1, pixfmt="yuyv")
    assert again()
    n, ptrs, ws, hs, _fmt, _keep = hipdrv._image_args(imgs, "rgb24")
    assert L.yolo2_hip_run_images_pix_int8_host(h, ptrs, ws, hs, 0x1234, n, 2, rp) == hipdrv.YOLO2_ERROR
    assert b"pixel format" in L.yolo2_hip_last_error()
    assert again()
    assert L.yolo2_hip_run_images_pix_int8_host(h, ptrs, ws, hs, hipdrv.PIXFMTS["rgb24"], 0, 2, rp) == hipdrv.YOLO2_ERROR
    assert again()
    holes = (hipdrv.C.c_void_p * 2)(ptrs[0], None)
    assert L.yolo2_hip_run_images_pix_int8_host(h, holes, ws, hs, hipdrv.PIXFMTS["rgb24"], 2, 2, rp) == hipdrv.YOLO2_ERROR
    assert b"null image 1" in L.yolo2_hip_last_error()
    assert again()
    with pytest.raises(hipdrv.Yolo2HipError, match="threshold"):
        hipdrv.run_images_dets(h, imgs, 2, -0.5, 0.45, precision="int8")
    assert again()


# ------------------------------------------------------------------ 8. neighbours on one context

def test_other_entries_on_the_same_context_are_unchanged():
    model = synth.SynthModel(seed=1)
    imgs = IMGS["rgb24"][1:4]
    frames = np.stack([hipdrv.letterbox_pix(im, "rgb24") for im in imgs])
    ctx = hipdrv.Yolo2Hip(0)
    try:
        ctx.load_model(model)
        ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
        ctx.load_model(ctx.calibrate_int8(frames=synth.frames(40, 2), batch=2))

        def neighbours():
            a = hipdrv.run_images_dets(ctx._h, imgs, 2, 0.05, 0.45, cap=845)
            b = hipdrv.run_images_dets(ctx._h, imgs, 2, 0.05, 0.45, cap=845, precision="fp16")
            return a, b, ctx.run_batch_int8_host(frames)

        a0, b0, r0 = neighbours()
        got = ctx.run_images_int8_host(imgs, 2)
        a1, b1, r1 = neighbours()
        assert _same_bits(got, r0) and _same_bits(r0, r1)
        assert a0["final_q"] == a1["final_q"]
        for x, y in ((a0, a1), (b0, b1)):
            assert np.array_equal(x["counts"], y["counts"])
            assert all(_records_equal(x["dets"][f], y["dets"][f]) for f in range(len(imgs)))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. memory

def test_images_route_frees_everything_and_never_holds_the_front_tensors(netw):
    imgs = IMGS["rgb24"][3:5]
    frames = np.stack([hipdrv.letterbox_pix(im, "rgb24") for im in imgs])
    start = hipdrv.live_bytes()
    ctx = hipdrv.Yolo2Hip(0)
    cal = netw.cal
    ctx.load_weights_int8(cal.w8, cal.bias32, cal.weight_q, cal.act_q)
    ctx.run_images_int8_host(imgs, 2)
    ctx.close()
    assert hipdrv.live_bytes() == start
    ctx = hipdrv.Yolo2Hip(0)
    try:
        ctx.load_weights_int8(cal.w8, cal.bias32, cal.weight_q, cal.act_q)
        a = ctx.run_images_int8_host(imgs, 2)
        d0 = hipdrv.live_bytes()[0]
        b = ctx.run_batch_int8_host(frames)
        d1 = hipdrv.live_bytes()[0]
        assert _same_bits(a, b)
        assert d1 - d0 >= 2 * 2 * 416 * 416 * 32, (d0, d1)
        assert _same_bits(ctx.run_images_int8_host(imgs, 2), a)
    finally:
        ctx.close()
    assert hipdrv.live_bytes() == start


# ------------------------------------------------------------------ 10. the command line

PKG = hipdrv.PKG_DIR
CLI = os.path.join(PKG, "yolov2_detect")


def _cli(args, cwd):
    return subprocess.run([CLI, "--cfg", os.path.join(PKG, "config", "yolov2.cfg"), "--names", os.path.join(PKG, "config", "coco.names")] + args,
                          capture_output=True, text=True, cwd=str(cwd), env=dict(os.environ, YOLO2_NO_DUMP="1"))


def _assert_jsonl_equals(recs, lib, imgs, thresh):
    total = 0
    assert len(recs) == len(imgs)
    for k, rec in enumerate(recs):
        assert (rec["width"], rec["height"]) == (imgs[k].shape[1], imgs[k].shape[0])
        want = [d for d in lib["dets"][k] if d["prob"] > thresh]
        got = rec["detections"]
        assert len(got) == len(want), k
        for g, w in zip(got, want):
            assert g["class_id"] == int(w["cls"])
            assert g["prob"] == float("%.6f" % w["prob"])
            assert [g["bbox_norm"][c] for c in "xywh"] == [float("%.6f" % w[c]) for c in "xywh"]
        total += len(got)
    return total


def test_cli_streams_on_the_int8_pass(netw, tmp_path):
    from yuyvref import formula, rgb_to_yuyv
    images = np.load(os.path.join(orclib.ROOT, "tests", "golden", "images.npz"))
    names = ["jpg/base_444", "png/rgb"]                            # the two files of test_calibrate_and_detect_tools_run_the_int8_set
    idir = tmp_path / "imgs"
    idir.mkdir()
    for k, name in enumerate(names):
        (idir / f"{k:02d}_{name.replace('/', '_')}.{name.split('/')[0]}").write_bytes(images[name + "/file"].tobytes())
    netw.cal.write_files(str(tmp_path / "int8"))
    thresh, nms = 0.005, 0.45
    common = ["--weights", str(tmp_path / "int8"), "--precision", "int8", "--batch", "2", "--thresh", str(thresh), "--nms", str(nms), "--post", "gpu"]
    out = tmp_path / "dir.jsonl"
    r = _cli(common + ["--input-dir", str(idir), "--jsonl", str(out)], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Streaming inference completed successfully (2 inference frames" in r.stdout
    imgs = [images[n + "/rgb"] for n in names]
    lib = hipdrv.run_images_dets(netw.ctx._h, imgs, 2, thresh, nms, cap=845, best_class=True, precision="int8")
    assert _assert_jsonl_equals([json.loads(line) for line in out.read_text().splitlines()], lib, imgs, thresh) > 0
    # a raw YUYV stream gives the records of the RGB24 stream of the converted frames
    rng = np.random.default_rng(3)
    w, h = 64, 48
    yuyv = [rgb_to_yuyv(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(3)]
    rgb = [formula(f) for f in yuyv]
    (tmp_path / "video.yuv").write_bytes(b"".join(f.tobytes() for f in yuyv))
    (tmp_path / "video.rgb").write_bytes(b"".join(f.tobytes() for f in rgb))
    got = {}
    for fmt, spelled in (("rgb", "rgb24"), ("yuv", "yuyv422")):
        path = tmp_path / f"video_{fmt}.jsonl"
        r = _cli(common + ["--video-raw", str(tmp_path / f"video.{fmt}"), "--video-pix-fmt", spelled, "--video-width", str(w), "--video-height", str(h),
                           "--jsonl", str(path)], tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[fmt] = [json.loads(line) for line in path.read_text().splitlines()]
    drop_source = lambda recs: [{k: v for k, v in rec.items() if k != "source"} for rec in recs]      # (the file's name)
    assert len(got["yuv"]) == 3 and drop_source(got["yuv"]) == drop_source(got["rgb"])
    lib = hipdrv.run_images_dets(netw.ctx._h, yuyv, 2, thresh, nms, cap=845, best_class=True, precision="int8", pixfmt="yuyv")
    _assert_jsonl_equals(got["yuv"], lib, yuyv, thresh)
    for extra in (["--devices", "0,1"], ["--loop-gpu", "--annotate-gpu", "--save-annotated-dir", str(tmp_path / "ann")]):
        r = _cli(common + ["--input-dir", str(idir)] + extra, tmp_path)
        assert r.returncode != 0 and "have no int8 form" in r.stderr, extra
