"""CPU tests of the edge-class pixel tiles of the int16 3x3 conv (conv_common.hpp): the partition the kernel decodes, replayed
on the host through yolo2_hip_i16_edge_map.  Every real pixel lies in exactly one tile, every tile runs every tap that is inside
the image for any of its pixels, and the step total is the closed form."""
import ctypes

import numpy as np
import pytest

from yolo2_amd import hipdrv

# tap (i, j) -> bit 3i + j; (dy, dx) = (i - 1, j - 1)
TOP, BOTTOM, LEFT, RIGHT, INTERIOR, MIXED = range(6)


def _edge_map(B, H, W):
    L = hipdrv.lib()
    nt = L.yolo2_hip_i16_edge_map(B, H, W, 0, None, None, None, None)
    assert nt >= 0
    if nt == 0:
        return None
    cls = np.zeros(nt, np.int32)
    mask = np.zeros(nt, np.int32)
    pix = np.zeros(nt * 64, np.int32)
    steps = ctypes.c_longlong(0)
    got = L.yolo2_hip_i16_edge_map(B, H, W, nt, cls.ctypes.data_as(ctypes.c_void_p), mask.ctypes.data_as(ctypes.c_void_p),
                                   pix.ctypes.data_as(ctypes.c_void_p), ctypes.byref(steps))
    assert got == nt
    return cls, mask, pix.reshape(nt, 64), steps.value


def _needed_taps(H, W, y, x):
    """Bit mask of the taps that are inside the image for the pixels (y, x) (arrays)."""
    m = np.zeros(y.shape, np.int32)
    for i in range(3):
        for j in range(3):
            yy, xx = y + i - 1, x + j - 1
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            m |= np.where(inside, 1 << (3 * i + j), 0)
    return m


@pytest.mark.parametrize("B", [1, 3, 21, 22, 64, 256])
def test_edge_partition_covers_once_and_keeps_every_inside_tap(B):
    sizes = [3, 4, 5, 13, 26, 52, 104]
    for H in sizes:
        for W in sizes:
            if B * H * W > 800_000 and H != W:
                continue   # (the square large maps are the network's; H != W is covered at the smaller sizes and batches)
            r = _edge_map(B, H, W)
            assert r is not None, (B, H, W)
            cls, mask, pix, steps = r
            npix = B * H * W
            real = pix[pix >= 0]
            # every real pixel in exactly one tile
            assert real.size == npix and np.array_equal(np.bincount(real, minlength=npix), np.ones(npix, np.int64)), (B, H, W)
            # only the last tile has padding lanes, and only a mixed tile
            pad_tiles = np.nonzero((pix < 0).any(axis=1))[0]
            assert pad_tiles.size <= 1 and all(cls[t] == MIXED for t in pad_tiles)
            # every tile's tap set contains every inside tap of each of its pixels
            q = np.where(pix >= 0, pix, 0)
            y, x = (q // W) % H, q % W
            need = np.where(pix >= 0, _needed_taps(H, W, y, x), 0)
            assert not np.any(need & ~mask[:, None]), (B, H, W)
            # class tiles hold only pixels of their class
            band = {TOP: y == 0, BOTTOM: y == H - 1, LEFT: (x == 0) & (y > 0) & (y < H - 1),
                    RIGHT: (x == W - 1) & (y > 0) & (y < H - 1), INTERIOR: (x > 0) & (x < W - 1) & (y > 0) & (y < H - 1)}
            for c, where in band.items():
                assert np.all(where[cls == c]), (B, H, W, c)
            assert np.array_equal(mask, np.array([0x1f8, 0x03f, 0x1b6, 0x0db, 0x1ff, 0x1ff])[cls])
            # the step total: 6 taps per full class tile of a band, 9 per interior and mixed tile, padding lanes included
            n = [B * W, B * W, B * (H - 2), B * (H - 2), B * (H - 2) * (W - 2)]
            mixed = -(-sum(v % 64 for v in n) // 64)
            closed = 64 * (6 * sum(v // 64 for v in n[:4]) + 9 * (n[4] // 64 + mixed))
            assert steps == closed == int(64 * np.array([bin(m).count("1") for m in mask]).sum()), (B, H, W)
            assert len(cls) == sum(v // 64 for v in n) + mixed


def test_edge_partition_interleaves_band_tiles():
    """The 6-tap band tiles are spread evenly over the grid (every contiguous eighth of it gets its share)."""
    cls, _, _, _ = _edge_map(21, 13, 13)
    band = cls < INTERIOR
    parts = np.array_split(band, 8)
    share = band.mean()
    for p in parts:
        assert abs(p.mean() - share) <= 1.0 / len(p) + 1e-9


def test_edge_partition_refuses_degenerate_maps():
    L = hipdrv.lib()
    for B, H, W in ((4, 2, 13), (4, 13, 2), (1, 1, 1)):
        assert L.yolo2_hip_i16_edge_map(B, H, W, 0, None, None, None, None) == 0


def test_edge_partition_step_saving_at_the_network_sizes():
    """The saving the issue predicts for the batch-64 lane sizes (21 / 22 frames): 6.8 - 8.3 % of the steps on 13x13."""
    for B in (21, 22):
        r = _edge_map(B, 13, 13)
        full = 9 * 64 * -(-B * 169 // 64)
        assert 0.068 <= 1 - r[3] / full <= 0.085, (B, 1 - r[3] / full)
