#!/usr/bin/env python3
"""Generate tests/golden/jpeg.npz from the REFERENCE's own JPEG writer.

Run in the build container only (needs /root/reference and gcc):
    python3 tests/golden/make_jpeg_golden.py

The reference's MJPEG streamer encodes every annotated frame with stbi_write_jpg_to_func(..., 3, rgb, quality)
(linux_app/src/yolo2_mjpeg_server.c:221-238; the vendored writer is stb_image_write v1.09).  This script compiles
linux_app/src/stb_image_write_impl.c into a temporary directory outside the repository, calls that function through ctypes and
stores DATA only: the input frames, their qualities and the bytes the reference wrote.  Nothing of the reference's program text
or binaries enters the repository.

Before writing, the script parses every stream's scan with the small decoder below and asserts that each situation the encoders
must get right occurs in some case: a sixteen-zeros code, a block without end-of-block, a DC difference of 0, a stuffed 0xFF, a
byte-aligned end, a filled last byte that is 0xFF, ragged widths and heights, AC category 10, DC category 11.

Keys: names (the case names); per case <name>/rgb uint8 [h][w][3], <name>/quality int32, <name>/jpg uint8 [n].
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_APP = "/root/reference/linux_app"
HEADER = 607


def build_ref(tmp):
    so = os.path.join(tmp, "libref_jpg.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I" + os.path.join(REF_APP, "include", "third_party"), "-o", so,
                    os.path.join(REF_APP, "src", "stb_image_write_impl.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    cb_t = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)
    lib.stbi_write_jpg_to_func.argtypes = [cb_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.stbi_write_jpg_to_func.restype = C.c_int

    def encode(rgb, quality):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, _ = rgb.shape
        parts = []
        cb = cb_t(lambda ctx, data, size: parts.append(C.string_at(data, size)))
        # the streamer's clamp (yolo2_mjpeg_server.c:224-225)
        assert lib.stbi_write_jpg_to_func(cb, None, w, h, 3, rgb.ctypes.data_as(C.c_void_p), min(max(int(quality), 1), 100)) == 1
        return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return encode


def huffman_tables(head):
    """the DHT segment of a stream's header -> {table id: {(length, code): symbol}}"""
    at = head.index(b"\xff\xc4")
    end = at + 2 + int.from_bytes(head[at + 2:at + 4], "big")
    at += 4
    tables = {}
    while at < end:
        tid, counts = head[at], head[at + 1:at + 17]
        at += 17
        code, t = 0, {}
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                t[(length, code)] = head[at]
                code += 1
                at += 1
            code <<= 1
        tables[tid] = t
    return tables


def scan_facts(jpg, w, h):
    """decode the scan of a reference stream; returns the set of situations met"""
    data = bytes(jpg)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and data[HEADER - 14:HEADER - 12] == b"\xff\xda"
    tables = huffman_tables(data[:HEADER])
    scan = data[HEADER:-2]
    facts = set()
    if b"\xff\x00" in scan[:-2]:
        facts.add("stuffed_ff")
    raw = scan.replace(b"\xff\x00", b"\xff")
    bits = "".join(f"{b:08b}" for b in raw)
    pos = 0

    def symbol(t):
        nonlocal pos
        code = 0
        for length in range(1, 17):
            code = (code << 1) | int(bits[pos + length - 1])
            if (length, code) in t:
                pos += length
                return t[(length, code)]
        raise AssertionError("no code")

    def value(cat):
        nonlocal pos
        if cat == 0:
            return 0
        v = int(bits[pos:pos + cat], 2)
        pos += cat
        return v if v >> (cat - 1) else v - (1 << cat) + 1

    for _ in range(((w + 7) // 8) * ((h + 7) // 8)):
        for comp in range(3):
            dc, ac = tables[0x00 if comp == 0 else 0x01], tables[0x10 if comp == 0 else 0x11]
            cat = symbol(dc)
            value(cat)
            if cat == 0:
                facts.add("dc_diff_0")
            if cat == 11:
                facts.add("dc_cat_11")
            k = 1
            while k < 64:
                s = symbol(ac)
                if s == 0x00:
                    break
                if s == 0xF0:
                    facts.add("zrl")
                    k += 16
                    continue
                k += s >> 4
                if (s & 15) == 10:
                    facts.add("ac_cat_10")
                assert (s & 15) <= 10
                value(s & 15)
                if k == 63:
                    facts.add("no_eob")
                k += 1
    assert len(bits) - pos < 8 and set(bits[pos:]) <= {"1"}, "the scan does not end where the blocks end"
    if pos % 8 == 0:
        assert len(bits) == pos
        facts.add("aligned_end")
    elif data[-4:] == b"\xff\x00\xff\xd9":
        facts.add("filled_byte_ff")
    if w % 8:
        facts.add("ragged_w")
    if h % 8:
        facts.add("ragged_h")
    return facts


def seeded(seed):
    """the draw order the rare stream ends were found with"""
    rng = np.random.default_rng(seed)
    w = int(rng.integers(1, 25))
    h = int(rng.integers(1, 25))
    q = int(rng.choice([1, 20, 50, 80, 95, 100]))
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), q


def cases():
    out = []
    rng = np.random.default_rng(20261019)
    for w, h, q in ((1, 1, 80), (8, 8, 80), (9, 7, 80), (64, 48, 80), (33, 17, 50), (40, 24, 100), (24, 40, 1), (97, 3, 90), (5, 211, 30)):
        out.append((f"rand_{w}x{h}_q{q}", rng.integers(0, 256, (h, w, 3)).astype(np.uint8), q))
    for seed, (w, h, q) in ((12, (15, 7, 100)), (14, (4, 20, 80)), (15, (23, 17, 95))):
        rgb, quality = seeded(seed)
        assert rgb.shape == (h, w, 3) and quality == q, (seed, rgb.shape, quality)
        out.append((f"seed{seed}_{w}x{h}_q{q}", rgb, q))
    dog = np.load(os.path.join(HERE, "dog.npz"))["rgb"]
    small = np.rint(dog.reshape(72, 8, 96, 8, 3).astype(np.float64).mean(axis=(1, 3))).astype(np.uint8)   # 768x576 -> 96x72, box filter
    out.append(("dog_96x72_q80", small, 80))
    out.append(("grey_16x16_q80", np.full((16, 16, 3), 128, dtype=np.uint8), 80))
    yy, xx = np.mgrid[0:16, 0:16]
    bw = lambda m: np.repeat((m.astype(np.uint8) * 255)[:, :, None], 3, axis=2)
    out.append(("checker_16x16_q100", bw((xx + yy) % 2 == 1), 100))
    out.append(("stripes_16x16_q100", bw(xx % 2 == 1), 100))
    out.append(("blocks_16x16_q100", bw(((xx // 8) + (yy // 8)) % 2 == 1), 100))
    return out


def main():
    if not os.path.isdir(REF_APP):
        sys.exit("needs the reference tree at " + REF_APP)
    out = {}
    names = []
    seen = {}
    with tempfile.TemporaryDirectory(prefix="y2_jpeg_ref_") as tmp:
        encode = build_ref(tmp)
        for name, rgb, q in cases():
            jpg = encode(rgb, q)
            assert len(jpg) > HEADER + 2
            for fact in scan_facts(jpg, rgb.shape[1], rgb.shape[0]):
                seen.setdefault(fact, []).append(name)
            names.append(name)
            out[name + "/rgb"] = rgb
            out[name + "/quality"] = np.int32(q)
            out[name + "/jpg"] = jpg
    for fact in ("zrl", "no_eob", "dc_diff_0", "stuffed_ff", "aligned_end", "filled_byte_ff", "ragged_w", "ragged_h", "ac_cat_10", "dc_cat_11"):
        assert fact in seen, f"no case shows {fact}"
        print(f"{fact:15s} {', '.join(seen[fact][:4])}{' ...' if len(seen[fact]) > 4 else ''}")
    out["names"] = np.array(names)
    path = os.path.join(HERE, "jpeg.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
