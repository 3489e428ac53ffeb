"""GPU tests of the JPEG encoder's modes (options jpeg_subsample / jpeg_restart; csrc/kernels_jpeg.hpp "the modes"): every entry
that writes JPEG gives the bytes of y2h_write_jpg_rgb24_ex, the host encoder tests/test_jpeg420_host.py pins - never the code under
test.  With the options unset, tests/test_gpu_jpeg.py shows today's bytes unchanged."""
import os

import numpy as np
import pytest

import orclib
from drawref import host_draw
from jpeg420ref import DOG, SHAPES, frame, host_decode, mcus, restarts
from test_gpu_jpeg import _mixed_set
from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu
NAMES = [s.strip() for s in open(os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
C = hipdrv.C
host_jpg = hipdrv.write_jpg_host


@pytest.mark.parametrize("quality", [50, 100])
@pytest.mark.parametrize("kind", ["noise", "crop"])
@pytest.mark.parametrize("subsample", [0, 420])
@pytest.mark.parametrize("w,h", SHAPES)
def test_encode_equals_the_host_encoder(w, h, subsample, kind, quality):
    """1x1: one MCU, edges repeated both ways; 17x15: ragged, 2x1 MCUs in 4:2:0; 48x48 with R = 1: the marker index wraps past 7;
    320x240 in 4:2:0: 300 MCUs = 1800 blocks = 15 groups of 128 blocks (R = 7 divides neither 300 nor a group; R = 20 spans groups),
    in 4:4:4 1200 MCUs; with R = 1 there are 299 (1199) pads, some of zero bits, and at quality 100 markers right behind FF 00."""
    rgb = frame(kind, w, h)
    for R in restarts(w, h, subsample):
        want = host_jpg(rgb, quality, subsample, R)
        if (w, h, kind, quality) == (320, 240, "noise", 100):
            assert len(want) > 613 + 2 * 4096 + 2 + 3 * 1200      # the unstuffed scan is more than one segment of stage D, markers aside
            assert R != 1 or any(want[i:i + 3] == b"\xff\x00\xff" and 0xD0 <= want[i + 3] <= 0xD7 for i in range(613, len(want) - 4))
        if R >= mcus(w, h, subsample)[1]:      # DRI and no marker
            assert want[593:595] == b"\xff\xdd" and not any(bytes([0xFF, 0xD0 + k]) in want[613:] for k in range(8))
        got = hipdrv.jpeg_encode(rgb, quality, subsample=subsample, restart=R)
        assert len(got) == len(want) and got == want, R


def test_odd_addresses_small_capacities_and_guard_bytes():
    """64x48 in mode (420, 5): 12 MCUs, markers behind MCUs 5 and 10.  Capacities: exact, one short, inside the header, between the FF
    and the Dn of the first marker, 0.  Nothing at or beyond the capacity is written and the size is always the stream's."""
    L = hipdrv.lib()
    rgb = frame("noise", 64, 48)
    want = host_jpg(rgb, 80, 420, 5)
    n = len(want)
    at = want.index(b"\xff\xd0", 613)      # (FF D0 in the scan is the marker: an entropy FF is followed by 00)
    src = hipdrv.DevBuf(np.concatenate([np.zeros(3, dtype=np.uint8), rgb.reshape(-1)]))
    size = C.c_size_t(0)
    with hipdrv.jpeg_mode(None, 420, 5):
        for shift, cap in ((1, n), (3, n - 1), (5, 600), (7, at + 1), (2, 0)):
            dst = hipdrv.DevBuf(np.full(n + 128, 0xA5, dtype=np.uint8))
            rc = L.yolo2_hip_jpeg_encode_rgb24(src.addr + 3, 64, 48, 80, dst.addr + shift if cap else 0, cap, C.byref(size), None)
            out = dst.get(np.uint8, (n + 128,))
            dst.free()
            assert size.value == n, (shift, cap)
            assert rc == (0 if cap >= n else hipdrv.YOLO2_ERROR), (shift, cap)
            k = min(cap, n)
            assert out[shift:shift + k].tobytes() == want[:k], (shift, cap)
            assert (out[:shift] == 0xA5).all() and (out[shift + k:] == 0xA5).all(), (shift, cap)
    src.free()


def test_batched_entry_and_loop_under_the_options():
    """annotate_images on the mixed set of tests/test_gpu_jpeg.py (1x1 .. 320x240) in mode (420, 4) at batch 4 - nine frames, a ragged
    last chunk - equals host painter + host encoder; loop_images with JPEG out under the same options equals the annotate entry on
    the loop's own records."""
    frames, dets, counts = _mixed_set()
    want = [host_jpg(host_draw(frames[f], dets[f, :min(counts[f], 845)], .24, NAMES)[0], 80, 420, 4) for f in range(9)]
    ctx = hipdrv.Yolo2Hip(0)
    outs, _ = ctx.annotate_images(frames, dets, counts, 4, .24, labels=NAMES, jpeg_quality=80, jpeg_subsample=420, jpeg_restart=4)
    assert outs == want
    assert ctx.options() == ""      # the options were for that call
    ctx.load_model(synth.SynthModel(seed=1, obj_bias=2.0))
    images = [np.ascontiguousarray(DOG[::2, ::2]), np.ascontiguousarray(DOG[100:340, 200:520]), frame("noise", 33, 17)]
    r = ctx.loop_images(images, thresh=.1, labels=NAMES, jpeg_quality=70, batch=2, jpeg_subsample=420, jpeg_restart=4)
    again, _ = ctx.annotate_images(images, r["dets"], None, 2, .1, labels=NAMES, jpeg_quality=70, jpeg_subsample=420, jpeg_restart=4)
    assert sum(int(d) for d in r["drawn"]) > 0 and r["frames"] == again
    assert r["frames"][2] == host_jpg(host_draw(images[2], r["dets"][2], .1, NAMES)[0], 70, 420, 4)
    ctx.close()


def test_the_gpu_decoder_takes_a_lane_per_row_of_our_stream():
    """closure: 320x240 in mode (420, MCUs per row) has a restart interval per MCU row - jpeg_probe reads it back, and the GPU decoder
    gives each of the 15 a lane - and decodes on the GPU to the host decoder's pixels"""
    rgb = frame("crop", 320, 240)
    data = hipdrv.jpeg_encode(rgb, 80, subsample=420, restart=20)
    assert data == host_jpg(rgb, 80, 420, 20)
    info = hipdrv.jpeg_probe(data)
    assert info["gpu_decodable"] and (info["hmax"], info["vmax"]) == (2, 2) and info["restart_interval"] == mcus(320, 240, 420)[0] == 20
    ctx = hipdrv.Yolo2Hip(0)
    frames, status = ctx.jpeg_decode([data])
    ctx.close()
    assert status[0] == 0 and np.array_equal(frames[0], host_decode(data))
