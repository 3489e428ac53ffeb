"""What tests/test_jpegdec_split_host.py and tests/test_gpu_jpegdec_split.py share: streams written here from seeded noise (long codes,
no DRI; the small ones are too short to split)."""
import functools

import numpy as np

import jpegdec_cases as jc

NOISE = [(q, h, w) for q in (95, 10) for (h, w) in ((1, 1), (8, 8), (33, 17), (61, 97))]    # (h, w): 1x1, 8x8, 17x33, 97x61


@functools.lru_cache(maxsize=None)
def noise_streams():
    return tuple(jc.write_jpg(np.random.default_rng(300 + k).integers(0, 256, (h, w, 3), dtype=np.uint8), q) for k, (q, h, w) in enumerate(NOISE))
