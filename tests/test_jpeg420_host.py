"""CPU tests of the JPEG encoder's modes on the host (y2h_write_jpg_rgb24_ex, libyolo2_host.so; csrc/jpeg_tables.hpp "the modes"):
subsample = 420 and restart = R are the library's own definition - the reference's writer has neither - so what pins them is that mode
(0, 0) is the reference's stream, that every mode decodes with the host decoder (itself pinned to the reference's stb_image), that
restart markers change no coefficient, and that 4:2:0 costs the fidelity chroma averaging costs and no more.  The GPU tests expect
this encoder's bytes."""
import io

import numpy as np
import pytest

from jpeg420ref import DOG, SHAPES, frame, host_decode, mcus, restarts
from jpegref import CASES, case
from yolo2_amd import hipdrv

enc = hipdrv.write_jpg_host


@pytest.mark.parametrize("name", CASES)
def test_mode_0_0_is_the_reference_stream(name):
    rgb, quality, want = case(name)
    assert enc(rgb, quality, 0, 0) == enc(rgb, quality) == want


@pytest.mark.parametrize("subsample", [0, 420])
@pytest.mark.parametrize("w,h", SHAPES)
def test_every_mode_decodes_and_restart_markers_change_no_pixel(w, h, subsample):
    rgb = frame("noise", w, h)
    plain = enc(rgb, 100, subsample, 0)
    want = host_decode(plain)
    assert want.shape == (h, w, 3)
    assert plain[165] == (0x22 if subsample else 0x11) and b"\xff\xdd" not in plain[:607]
    n = mcus(w, h, subsample)[1]
    for R in restarts(w, h, subsample)[1:]:
        data = enc(rgb, 100, subsample, R)
        assert data[593:599] == bytes([0xFF, 0xDD, 0, 4, R >> 8, R & 255]) and data[599:601] == b"\xff\xda", R
        # the markers count up modulo 8, one per interval but the last; the scan holds FF only before 00 or a marker
        scan = data[613:-2]
        marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
        assert marks == [0xD0 + (k & 7) for k in range(-(-n // R) - 1)], R
        assert np.array_equal(host_decode(data), want), R
        assert len(data) <= hipdrv.host_lib().y2h_jpg_rgb24_bound_ex(w, h, subsample, R)


@pytest.mark.parametrize("subsample,restart", [(420, 0), (420, 3), (0, 3)])
def test_another_decoder_opens_the_streams(subsample, restart):
    Image = pytest.importorskip("PIL.Image")
    for w, h in SHAPES:
        im = Image.open(io.BytesIO(enc(frame("crop", w, h), 80, subsample, restart)))
        im.load()
        assert im.size == (w, h) and im.mode == "RGB"


def test_bad_modes_are_argument_errors():
    H = hipdrv.host_lib()
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)
    for subsample, restart in ((422, 0), (1, 0), (0, -1), (0, 65536), (420, 70000)):
        assert H.y2h_write_jpg_rgb24_ex(rgb.ctypes.data, 4, 4, 80, subsample, restart, None, 0) == -1
        assert H.y2h_jpg_rgb24_bound_ex(4, 4, subsample, restart) == 0
    # a 4:2:0 frame below 16 x 16 has more blocks than its 4:4:4 form; (0, 0) is the old bound
    assert H.y2h_jpg_rgb24_bound_ex(8, 8, 0, 0) == H.y2h_jpg_rgb24_bound(8, 8) == 607 + 2 * ((3 * 1660 + 7) // 8) + 2
    assert H.y2h_jpg_rgb24_bound_ex(8, 8, 420, 0) == 607 + 2 * ((6 * 1660 + 7) // 8) + 2
    assert H.y2h_jpg_rgb24_bound_ex(48, 48, 420, 2) == 613 + 2 * ((54 * 1660 + 7) // 8) + 3 * 5 + 2


def test_fidelity_of_420_on_the_dog_frame():
    """Mean absolute error against the source at quality 80, host encoder and host decoder (profiles/r23_jpeg420.txt): 4:4:4 2.660,
    4:2:0 3.077, ratio 1.157.  4:2:0 replaces each 2x2 of Cb and Cr by its mean, so its error must lie above the 4:4:4 one - below it
    means the chroma planes were not averaged - and a broken definition (wrong block order, shifted chroma) costs tens of levels.  The
    margin: the chroma planes carry at most half of an RGB error (|dR/dCr| = 1.402, |dB/dCb| = 1.772, G mostly from Y), and losing
    their upper half-band on a natural frame cannot double the whole error: 4:4:4 < 4:2:0 <= 1.5 x 4:4:4."""
    err = lambda data: float(np.abs(host_decode(data).astype(np.int32) - DOG).mean())
    e444, e420 = err(enc(DOG, 80, 0, 0)), err(enc(DOG, 80, 420, 0))
    print(f"dog q80: 4:4:4 {e444:.4f}, 4:2:0 {e420:.4f}, ratio {e420 / e444:.4f}")
    assert e444 < e420 <= 1.5 * e444
