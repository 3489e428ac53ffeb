"""GPU tests of the images entries on the matrix-core passes: yolo2_hip_run_images_u8_f16_host / _dets_f16 and the multi form.
Layers 0+1 read the image bytes themselves (k_conv0_pool_mfma_u8); the contract is bit identity with letterboxing every image
(yolo2_hip_letterbox_u8) and running the frame entries (run_batch_fp16 / _f32tol) on the same chunks, and - under the option
f16_no_mfma0, where the entries take the two-kernel route - with that option's frame path."""
import os

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
ROOT = orclib.ROOT
DOG = np.load(os.path.join(ROOT, "tests", "golden", "dog.npz"))
FUSED = {0: "k_conv0_pool_mfma_u8", 1: "k_conv0_pool_mfma_u8<split>"}


def _rgb_set():
    rgb = DOG["rgb"]
    return [rgb, rgb[::2, ::2].copy(), rgb[:, ::-1].copy(), rgb[100:400, 50:700].copy(), rgb.transpose(1, 0, 2).copy(),
            np.ascontiguousarray(np.tile(rgb[200:260], (1, 4, 1))),     # very wide: 3072 x 60
            rgb[300:301, 100:400].copy()]                                 # 300 x 1: a fitted height of 1


def _grey_set():
    g = DOG["rgb"][:, :, 1]
    return [g.copy(), g[::3, ::2].copy(), g[:200].T.copy()]


def _frames(images):
    return np.stack([hipdrv.letterbox_u8(im) for im in images])


def _frame_path(ctx, frames, batch, split):
    """the reference route: the frame entry on the same chunks (a partial last chunk repeats its last frame, as the entries do)"""
    run = ctx.run_batch_f32tol_host if split else ctx.run_batch_fp16_host
    out = []
    for k in range(0, len(frames), batch):
        chunk = frames[k:k + batch]
        pad = np.concatenate([chunk, np.repeat(chunk[-1:], batch - len(chunk), axis=0)]) if len(chunk) < batch else chunk
        out.append(run(pad)[:len(chunk)])
    return np.concatenate(out)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def model():
    return synth.SynthModel(seed=1)


@pytest.mark.parametrize("split", [0, 1])
def test_images_f16_bit_identical_to_letterbox_then_frame_path(model, split):
    rgb, grey = _rgb_set(), _grey_set()
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    assert ctx.images_layer0_kernel(split) == ""
    frames_rgb, frames_grey = _frames(rgb), _frames(grey)
    for images, frames in ((rgb, frames_rgb), (grey, frames_grey)):
        for batch in (1, 3):
            got = ctx.run_images_f16_host(images, batch, split=bool(split))
            want = _frame_path(ctx, frames, batch, split)
            assert _same_bits(got, want), (split, batch, len(images))
            assert ctx.images_layer0_kernel(split) == FUSED[split]
    # batch 64: two lanes of 32, each lane's layer 0 starting at its own item of the chunk's table; 70 images = a ragged second chunk
    many = [rgb[k % len(rgb)] for k in range(70)]
    idx = [k % len(rgb) for k in range(70)]
    got = ctx.run_images_f16_host(many, 64, split=bool(split))
    want = _frame_path(ctx, frames_rgb[idx], 64, split)
    assert _same_bits(got, want)
    assert ctx.images_layer0_kernel(split) == FUSED[split]
    assert (ctx.num_lanes_f32tol() if split else ctx.num_lanes_fp16()) == 2
    ctx.close()


@pytest.mark.parametrize("split", [0, 1])
def test_images_f16_no_mfma0_takes_the_two_kernel_route(model, split):
    rgb = _rgb_set()
    ctx = hipdrv.Yolo2Hip(0)
    ctx.set_option("f16_no_mfma0", 1)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    got = ctx.run_images_f16_host(rgb, 3, split=bool(split))
    want = _frame_path(ctx, _frames(rgb), 3, split)
    assert _same_bits(got, want)
    name = ctx.images_layer0_kernel(split)
    assert name == "k_letterbox_u8_batch + " + ("k_conv0_pool_f16<split>" if split else "k_conv0_pool_f16")
    assert name.endswith(ctx.f32tol_layer_kernel(0) if split else hipdrv.lib().yolo2_hip_fp16_layer_kernel(ctx._h, 0).decode())
    ctx.close()


def _best_class(recs):
    exp = []
    for det in np.unique(recs["det"]):       # records are grouped by detection, classes ascending
        rows = recs[recs["det"] == det]
        exp.append(rows[np.argmax(rows["prob"])])
    return np.array(exp, dtype=recs.dtype)


@pytest.mark.parametrize("precision", ["fp16", "fp32fast"])
def test_images_f16_records_equal_postprocess_f32(model, precision):
    split = int(precision == "fp32fast")
    rgb = DOG["rgb"]           # the int16 entry's test set (test_gpu_post_multi.py)
    imgs = [rgb, rgb[::2, ::2].copy(), rgb[:, ::-1].copy(), rgb[100:400, 50:700].copy(), rgb.transpose(1, 0, 2).copy(), rgb[::3, ::2].copy(),
            rgb[:300].copy()]
    thresh, nms = 0.05, 0.45
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    region = ctx.run_images_f16_host(imgs, 3, split=bool(split))
    buf = hipdrv.DevBuf(np.ascontiguousarray(region))
    ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
    want = hipdrv.postprocess(ctx, buf.addr, len(imgs), ws, hs, thresh, nms, cap=4096)
    buf.free()
    assert min(int(c) for c in want["counts"]) > 5, want["counts"]
    for batch in (2, 3):
        got = hipdrv.run_images_dets(ctx._h, imgs, batch, thresh, nms, cap=4096, best_class=False, precision=precision)
        assert np.array_equal(got["counts"], want["counts"])
        for f in range(len(imgs)):
            assert np.array_equal(got["dets"][f], want["dets"][f]), (batch, f)
    best = hipdrv.run_images_dets(ctx._h, imgs, 3, thresh, nms, cap=845, best_class=True, precision=precision)
    for f in range(len(imgs)):
        exp = _best_class(want["dets"][f])
        assert int(best["counts"][f]) == len(exp) <= 845
        assert np.array_equal(best["dets"][f], exp), f
        assert (best["dets"][f]["frame"] == f).all()
    ctx.close()
    m = hipdrv.Yolo2HipMulti([0, 0])
    m.load_model_fp32(model)
    gm = hipdrv.run_images_dets(m._m, imgs, 2, thresh, nms, cap=845, best_class=True, multi=True, precision=precision)
    m.close()
    assert np.array_equal(gm["counts"], best["counts"])
    for f in range(len(imgs)):
        assert np.array_equal(gm["dets"][f], best["dets"][f]), f


def _slots(region_f32):
    proc = np.zeros(425 * 169, dtype=np.float32)
    orclib.host().y2h_region_forward(np.ascontiguousarray(region_f32.reshape(-1)), proc)
    rows = np.zeros((845, 85), dtype=np.float32)
    orclib.host().y2h_boxes_nms(proc, 768, 576, 0.0, 0.0, rows, 845)   # no threshold, no NMS: every slot in cell/anchor order
    return rows


def _iou(a, b):
    l = np.maximum(a[:, 0] - a[:, 2] / 2, b[:, 0] - b[:, 2] / 2); r = np.minimum(a[:, 0] + a[:, 2] / 2, b[:, 0] + b[:, 2] / 2)
    t = np.maximum(a[:, 1] - a[:, 3] / 2, b[:, 1] - b[:, 3] / 2); d = np.minimum(a[:, 1] + a[:, 3] / 2, b[:, 1] + b[:, 3] / 2)
    inter = np.clip(r - l, 0, None) * np.clip(d - t, 0, None)
    return inter / (a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3] - inter)


def test_images_f16_dog_within_tolerance_of_the_fp32_reference(model):
    """dog.jpg's bytes through both entries against the compiled reference's fp32 region tensor of the same image: the split pass
    within 1e-3 (raw tensor and all four coordinates of every one of the 845 slots), the fp16 pass within the fp16 bounds."""
    ref = DOG["f32/region_raw_f32"].reshape(425, 13, 13)
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    tol = ctx.run_images_f16_host([DOG["rgb"]], 1, split=True)[0]
    assert np.abs(tol - ref).max() <= 1e-3
    ra, ga = _slots(ref), _slots(tol)
    assert (ra[:, 2] > 0).all() and (ga[:, 2] > 0).all()
    assert np.abs(ga[:, :4] - ra[:, :4]).max() <= 1e-3
    f16 = ctx.run_images_f16_host([DOG["rgb"]], 1, split=False)[0]
    g16 = _slots(f16)
    assert np.abs(g16[:, :4] - ra[:, :4]).max() <= 1e-2
    iou = _iou(g16, ra)
    assert iou.min() >= 0.93 and iou.mean() >= 0.99, (iou.min(), iou.mean())
    ctx.close()


def test_images_f16_errors(model):
    L = hipdrv.lib()
    rgb = DOG["rgb"]
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(model)                       # int16 weights only
    for split in (0, 1):
        with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
            ctx.run_images_f16_host([rgb], 1, split=bool(split))
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        hipdrv.run_images_dets(ctx._h, [rgb], 1, 0.05, 0.45, precision="fp16")
    ctx.close()
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    n, ptrs, ws, hs, ch, keep = hipdrv._image_args([rgb, rgb])
    out = np.zeros((2, 425, 13, 13), dtype=np.float32)
    dets = np.zeros((2, 8), dtype=hipdrv.DET_DTYPE)
    counts = np.zeros(2, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(hipdrv.C.c_void_p)
    host = lambda *a: L.yolo2_hip_run_images_u8_f16_host(ctx._h, *a)
    cases = [
        (host(0, ptrs, ws, hs, 2, n, 1, vp(out)), "geometry"),         # channels 2
        (host(0, ptrs, ws, hs, 4, n, 1, vp(out)), "geometry"),         # channels 4
        (host(0, ptrs, ws, hs, ch, 0, 1, vp(out)), "image count"),     # n 0
        (host(0, ptrs, ws, hs, ch, n, 0, vp(out)), "image count"),     # batch 0
        (host(0, None, ws, hs, ch, n, 1, vp(out)), "null"),
        (host(0, ptrs, ws, hs, ch, n, 1, None), "null"),
        (host(2, ptrs, ws, hs, ch, n, 1, vp(out)), "split"),
        (host(0, ptrs, (hipdrv.C.c_int * 2)(0, 768), hs, ch, n, 1, vp(out)), "geometry"),
        (L.yolo2_hip_run_images_u8_dets_f16(ctx._h, 0, ptrs, ws, hs, ch, n, 1, 0.05, 0.45, 0, vp(dets), 0, vp(counts)), "capacity"),
        (L.yolo2_hip_run_images_u8_dets_f16(ctx._h, 1, ptrs, ws, hs, ch, n, 1, 0.05, 0.45, 0, None, 8, vp(counts)), "null"),
        (L.yolo2_hip_run_images_u8_dets_f16(None, 0, ptrs, ws, hs, ch, n, 1, 0.05, 0.45, 0, vp(dets), 8, vp(counts)), "null"),
    ]
    for rc, what in cases:
        assert rc == hipdrv.YOLO2_ERROR, what
    null_img = (hipdrv.C.c_void_p * 2)(ptrs[0], None)
    assert host(0, null_img, ws, hs, ch, n, 1, vp(out)) == hipdrv.YOLO2_ERROR
    assert b"null image" in L.yolo2_hip_last_error()
    assert L.yolo2_hip_run_images_u8_f16_host(ctx._h, 0, ptrs, ws, hs, 2, n, 1, vp(out)) == hipdrv.YOLO2_ERROR
    assert b"geometry" in L.yolo2_hip_last_error()
    assert ctx.images_layer0_kernel(0) == "" and ctx.images_layer0_kernel(1) == ""    # nothing ran
    # the context still works after the refusals
    got = ctx.run_images_f16_host([rgb], 1)
    assert _same_bits(got, ctx.run_batch_fp16_host(_frames([rgb])))
    ctx.close()
    m = hipdrv.Yolo2HipMulti([0, 0])
    m.load_model(model)
    with pytest.raises(hipdrv.Yolo2HipError, match="fp32 weights not loaded"):
        hipdrv.run_images_dets(m._m, [rgb, rgb], 1, 0.05, 0.45, multi=True, precision="fp32fast")
    m.close()
