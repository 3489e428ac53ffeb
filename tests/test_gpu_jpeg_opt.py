"""GPU tests of the JPEG encoder's optimize mode (option jpeg_optimize; csrc/kernels_jpeg.hpp "optimize"): every entry that writes
JPEG gives the bytes of y2h_write_jpg_rgb24_opt, the host encoder tests/test_jpeg_opt_host.py pins - never the code under test.  With
the option unset the bytes are those of tests/test_gpu_jpeg.py and tests/test_gpu_jpeg420.py."""
import os

import numpy as np
import pytest

import orclib
from drawref import host_draw
from jpeg420ref import DOG, frame, host_decode
from test_jpeg_opt_host import FRAMES, MODES, opt_frame
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
NAMES = [s.strip() for s in open(os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
C = hipdrv.C
host_jpg = hipdrv.write_jpg_host


@pytest.mark.parametrize("quality", [50, 80, 100])
@pytest.mark.parametrize("subsample,restart", MODES)
@pytest.mark.parametrize("name", FRAMES + ["fade"])
def test_encode_equals_the_host_encoder(name, subsample, restart, quality):
    rgb = opt_frame(name)
    got = hipdrv.jpeg_encode(rgb, quality, subsample=subsample, restart=restart, optimize=True)
    assert got == host_jpg(rgb, quality, subsample, restart, optimize=True)


def test_unset_after_set_gives_the_standard_bytes():
    rgb = frame("crop", 48, 32)
    assert hipdrv.jpeg_encode(rgb, 80, optimize=True) != host_jpg(rgb, 80)
    assert hipdrv.jpeg_encode(rgb, 80) == host_jpg(rgb, 80)
    assert hipdrv.jpeg_encode(rgb, 80, subsample=420, restart=4) == host_jpg(rgb, 80, 420, 4)


@pytest.mark.parametrize("subsample,restart", [(0, 0), (420, 4)])
def test_a_chunk_of_unlike_frames_with_a_fallback_frame(subsample, restart):
    """one chunk: per-frame tables, per-frame header lengths (267 .. 600 bytes) and - quality 100 - the frame past kOptCountLimit in
    4:4:4, which is the standard stream, side by side; no records, so the painter leaves the frames as they are"""
    names = ["noise33x31", "big", "1x1", "fade", "crop17x9"]
    images = [opt_frame(n) for n in names]
    ctx = hipdrv.Yolo2Hip(0)
    outs, _ = ctx.annotate_images(images, [np.zeros(0, dtype=hipdrv.DET_DTYPE)] * 5, None, 5, .24, jpeg_quality=100, jpeg_subsample=subsample,
                                  jpeg_restart=restart, jpeg_optimize=1)
    assert ctx.options() == ""      # the options were for that call
    ctx.close()
    for n, im, out in zip(names, images, outs):
        assert out == host_jpg(im, 100, subsample, restart, optimize=True), n
    assert (outs[1] == host_jpg(images[1], 100, subsample, restart)) == (subsample == 0)


def test_small_capacities_and_guard_bytes():
    """48x32 in mode (420, 4) with its own tables: capacities exact, one short, inside the DHT segment, 0.  Nothing at or beyond the
    capacity is written and the size is always the stream's."""
    L = hipdrv.lib()
    rgb = frame("crop", 48, 32)
    want = host_jpg(rgb, 80, 420, 4, optimize=True)
    n = len(want)
    src = hipdrv.DevBuf(np.concatenate([np.zeros(3, dtype=np.uint8), rgb.reshape(-1)]))
    size = C.c_size_t(0)
    with hipdrv.jpeg_mode(None, 420, 4, optimize=1):
        for shift, cap in ((1, n), (3, n - 1), (5, 200), (2, 0)):
            dst = hipdrv.DevBuf(np.full(n + 128, 0xA5, dtype=np.uint8))
            rc = L.yolo2_hip_jpeg_encode_rgb24(src.addr + 3, 48, 32, 80, dst.addr + shift if cap else 0, cap, C.byref(size), None)
            out = dst.get(np.uint8, (n + 128,))
            dst.free()
            assert size.value == n and rc == (0 if cap >= n else hipdrv.YOLO2_ERROR), (shift, cap)
            k = min(cap, n)
            assert out[shift:shift + k].tobytes() == want[:k], (shift, cap)
            assert (out[:shift] == 0xA5).all() and (out[shift + k:] == 0xA5).all(), (shift, cap)
    src.free()


def test_annotate_and_both_loops_under_the_option():
    """the annotate entry on painted frames equals host painter + host encoder; loop_images and loop_jpegs with JPEG out under the
    option equal the host encoder on the host-painted frames of their own records"""
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(synth.SynthModel(seed=1, obj_bias=2.0))
    images = [np.ascontiguousarray(DOG[::2, ::2]), np.ascontiguousarray(DOG[100:340, 200:520]), frame("noise", 33, 17)]
    kw = dict(thresh=.1, labels=NAMES, jpeg_quality=70, batch=2, jpeg_subsample=420, jpeg_restart=4, jpeg_optimize=1)
    want = lambda ims, r: [host_jpg(host_draw(im, d, .1, NAMES)[0], 70, 420, 4, optimize=True) for im, d in zip(ims, r["dets"])]
    r = ctx.loop_images(images, **kw)
    assert sum(int(d) for d in r["drawn"]) > 0 and r["frames"] == want(images, r)
    again, _ = ctx.annotate_images(images, r["dets"], None, 2, .1, labels=NAMES, jpeg_quality=70, jpeg_subsample=420, jpeg_restart=4, jpeg_optimize=1)
    assert again == r["frames"]
    streams = [host_jpg(im, 90, 420, 8, optimize=True) for im in images[:2]]      # (the GPU decoder wants even sizes)
    rj = ctx.loop_jpegs(streams, **kw)
    assert not rj["status"].any() and rj["frames"] == want([host_decode(s) for s in streams], rj)
    assert ctx.options() == ""
    ctx.close()


@pytest.mark.parametrize("restart", [0, 20])
def test_the_gpu_decoder_takes_the_optimised_stream(restart):
    rgb = frame("crop", 320, 240)
    data = hipdrv.jpeg_encode(rgb, 80, subsample=420, restart=restart, optimize=True)
    assert data == host_jpg(rgb, 80, 420, restart, optimize=True) and hipdrv.jpeg_probe(data)["gpu_decodable"]
    ctx = hipdrv.Yolo2Hip(0)
    frames, status = ctx.jpeg_decode([data])
    ctx.close()
    assert status[0] == 0 and np.array_equal(frames[0], host_decode(data))
