#!/usr/bin/env python3
"""Generate tests/golden/draw.npz from the REFERENCE's own annotated-frame painter.

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_draw_golden.py

The reference's camera / video loop ends every frame with yolo2_draw_detections_rgb24 (linux_app/src/yolo2_draw.c:276-369, called at
linux_app/src/main.c:1079-1091): one box and a "<label> <prob>" tag per detection, painted into the RGB24 frame.  This script compiles
that translation unit from the reference's sources into a temporary directory OUTSIDE the repository, calls the function, and stores
only data: random-byte frames, records, label lists, thresholds, what the reference painted (the pixels that differ from the frame,
as a mask and their values: a few colours, which compress well where the random frame does not) and its return values; plus every
glyph of its font as the reference rendered it, 5 x 7 cells and the same as one 35-bit word each (bit 5 * row + column, column 0 on
the left).  tests/test_draw_host.py pins y2h_draw_detections_rgb24 and the host's packed font to it; the GPU tests take the restatement as their expected side at other sizes.

Before it writes the file the generator checks that every situation the cases are meant to hold really occurs.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_APP = "/root/reference/linux_app"
FONT_CHARS = " .0123456789abcdefghijklmnopqrstuvwxyz"   # the 38 characters with a glyph (A-Z share a-z's)


class Box(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float)]


class Det(C.Structure):
    _fields_ = [("bbox", Box), ("objectness", C.c_float), ("prob", C.POINTER(C.c_float)), ("classes", C.c_int), ("sort_class", C.c_int)]


def build_reference(tmp):
    so = os.path.join(tmp, "libref_draw.so")
    src = [os.path.join(REF_APP, "src", f) for f in ("yolo2_draw.c", "stb_image_write_impl.c")]
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I" + os.path.join(REF_APP, "include"),
                    "-I" + os.path.join(REF_APP, "include", "third_party"), "-o", so] + src + ["-lm"], check=True)
    lib = C.CDLL(so)
    lib.yolo2_draw_detections_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
    lib.yolo2_draw_detections_rgb24.restype = C.c_int
    return lib


def ref_draw(lib, frame, cls, box, thresh, labels):
    """frame uint8 [h][w][3]; cls int [n]; box float32 [n][5] = prob, x, y, w, h; labels: list of str or None -> (out, drawn)"""
    out = np.ascontiguousarray(frame, dtype=np.uint8).copy()
    h, w = out.shape[:2]
    n = len(cls)
    classes = max(80, int(max(cls, default=0)) + 1)
    probs = np.zeros((max(n, 1), classes), dtype=np.float32)
    dets = (Det * max(n, 1))()
    for i in range(n):
        probs[i, cls[i]] = box[i][0]
        dets[i].bbox = Box(*[float(v) for v in box[i][1:5]])
        dets[i].prob = probs[i].ctypes.data_as(C.POINTER(C.c_float))
        dets[i].classes = classes
    if labels is None:
        lab, nlab = None, 0
    else:
        enc = [s.encode() for s in labels]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        lab, nlab = C.cast(arr, C.c_void_p), len(enc)
    drawn = lib.yolo2_draw_detections_rgb24(out.ctypes.data, w, h, C.cast(dets, C.c_void_p), n, C.c_float(thresh), lab, nlab)
    return out, drawn


def corners(box, w, h):
    """the reference's corner arithmetic in fp32 (x86 cast semantics), after the clamp: x0, y0, x1, y1 and the raw values"""
    f = np.float32

    def cast(v):
        return int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2 ** 31

    with np.errstate(all="ignore"):
        _, x, y, bw, bh = [f(v) for v in box]
        raw = [cast((x - bw * f(.5)) * f(w)), cast((y - bh * f(.5)) * f(h)), cast((x + bw * f(.5)) * f(w)), cast((y + bh * f(.5)) * f(h))]
    lim = [w - 1, h - 1, w - 1, h - 1]
    return [min(max(v, 0), m) for v, m in zip(raw, lim)], raw


def main():
    if not os.path.isdir(REF_APP):
        sys.exit("needs the reference tree at /root/reference")
    rng = np.random.default_rng(20261019)
    names = [s.strip() for s in open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "config", "coco.names")) if s.strip()]
    cases = {}

    def case(name, w, h, recs, thresh, labels):
        cases[name] = dict(frame=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), cls=np.array([r[0] for r in recs], dtype=np.int32),
                           box=np.array([r[1:] for r in recs], dtype=np.float32).reshape(len(recs), 5), thresh=np.float32(thresh), labels=labels)

    # every glyph, upper case mapped to lower, and characters without a glyph ('_', '!'), two tags per 160 x 40 frame
    glyph_labels = ["abcdefgh", "ijklmnop", "qrstuvwx", "yz012345", "6789. AZ", "a_b!"]
    for k in range(3):
        case(f"glyphs{k}", 160, 40, [(2 * k, .5, .49, .25, .98, .5), (2 * k + 1, .25, .49, 1.0, .98, .05)], .1, glyph_labels)
    nan = float("nan")
    main_recs = [
        (0, .9, .3, .6, .3, .4),          # tag above the box
        (1, .8, .7, .3, .3, .4),          # y0 < 18: tag flipped below the box's top
        (2, .7, .05, .5, .3, .2),         # cut by the left edge
        (3, .7, .95, .5, .3, .2),         # cut by the right edge (and its tag runs off it)
        (4, .7, .5, .05, .2, .3),         # cut by the top edge
        (5, .7, .5, .95, .2, .3),         # cut by the bottom edge
        (6, .7, .8, .5, .1, .2),          # tag running off the right edge
        (7, .6, .4, .5, .3, .3), (8, .6, .5, .55, .3, .3),      # overlapping, A then B
        (8, .6, .3, .85, .2, .2), (7, .6, .25, .8, .2, .2),     # overlapping, B then A
        (7, .5, .5, .5, 0., .5),          # x0 == x1
        (8, .5, .6, .4, .4, 0.),          # y0 == y1
        (0, .5, .9, .9, 0., 0.),          # a point
        (1, .125, .2, .2, .1, .1), (2, .375, .6, .7, .1, .1), (3, .995, .1, .9, .1, .1),   # %.2f ties and carry
        (4, .1, .5, .5, .5, .5),          # at thresh: skipped
        (5, .05, .5, .5, .5, .5),         # below thresh: skipped
        (6, .9, .5, .5, 1e12, 1e12),      # products outside int range
        (7, .9, .5, .5, nan, .2),         # NaN width
        (0, .9, .7, .8, -.2, .1),         # negative width: x0 > x1
    ]
    case("main", 96, 64, main_recs, .1, names[:5])
    case("nolabels", 48, 24, [(3, .5, .5, .5, .5, .5)], .1, None)
    case("odd33x17", 33, 17, [(0, .9, .5, .5, .6, .6), (5, .9, .2, .9, .3, .3), (6, .4, 1., 0., .5, .5)], .1, names)
    case("one1x1", 1, 1, [(0, .9, .5, .5, 1., 1.)], .1, names)
    case("empty", 16, 8, [], .1, names)
    many = [(int(rng.integers(0, 80)), float(rng.uniform(.3, 1.)), float(rng.random()), float(rng.random()), float(rng.uniform(0, .1)),
             float(rng.uniform(0, .1))) for _ in range(845)]
    case("many845", 64, 48, many, .24, names)
    long_label = ("the quick brown fox jumps over 13 lazy dogs. " * 5)[:200]
    case("longlabel", 64, 24, [(0, .5, .1, .9, .1, .1)], .1, [long_label])

    with tempfile.TemporaryDirectory(prefix="y2_draw_ref_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        lib = build_reference(tmp)
        for c in cases.values():
            c["out"], c["drawn"] = ref_draw(lib, c["frame"], c["cls"], c["box"], float(c["thresh"]), c["labels"])
        # the font, one character per call on a black frame: class 0 gives white text at (2, 3), scale 2
        bitmaps = np.zeros((len(FONT_CHARS), 7, 5), dtype=np.uint8)
        blank = np.zeros((24, 80, 3), dtype=np.uint8)
        for i, ch in enumerate(FONT_CHARS + "_!A"):
            o, _ = ref_draw(lib, blank, [0], [(.5, 0., 0., 0., 0.)], .1, [ch])
            cell = (o[3:17, 2:12] == 255).all(axis=2)
            assert (cell[0::2, 0::2] == cell[1::2, 1::2]).all() and (cell[0::2, 0::2] == cell[0::2, 1::2]).all(), "scale-2 blocks"
            bm = cell[0::2, 0::2].astype(np.uint8)
            if i < len(FONT_CHARS):
                bitmaps[i] = bm
            elif ch == "A":
                assert (bm == bitmaps[FONT_CHARS.index("a")]).all(), "upper case maps to lower case"
            else:
                assert not bm.any(), f"{ch!r} renders as a blank"
    words = np.array([sum(int(b[r, c]) << (5 * r + c) for r in range(7) for c in range(5)) for b in bitmaps], dtype=np.uint64)
    assert not bitmaps[0].any() and all(b.any() for b in bitmaps[1:]) and len(set(words.tolist())) == len(FONT_CHARS) - 1, \
        "37 distinct non-blank glyphs (o and 0 share one) and the space"

    # ---- does every situation occur?
    m = cases["main"]
    geo = [corners(b, 96, 64) for b in m["box"]]
    used = [i for i, b in enumerate(m["box"]) if b[0] > m["thresh"]]
    assert m["drawn"] == len(used) == len(main_recs) - 2, "records at and below thresh are skipped"
    flipped = [geo[i][0][1] < 18 for i in used]
    assert any(flipped) and not all(flipped), "tags above and flipped"
    assert any(geo[i][1][0] < 0 for i in used) and any(geo[i][1][2] > 95 for i in used), "left / right cut"
    assert any(geo[i][1][1] < 0 for i in used) and any(geo[i][1][3] > 63 for i in used), "top / bottom cut"
    assert any(geo[i][0][0] + 100 > 95 for i in used), "a tag runs off the right edge"
    assert any(g[0][0] == g[0][2] and g[0][1] != g[0][3] for g in geo) and any(g[0][1] == g[0][3] and g[0][0] != g[0][2] for g in geo)
    assert set(int(c) % 8 for c in m["cls"][used]) == set(range(8)) and 8 in m["cls"][used], "every palette colour and the wrap"
    assert (m["cls"][used] >= len(m["labels"])).any(), "cls >= n_labels"
    assert geo[19][1] == [-2 ** 31] * 4 and geo[19][0] == [0, 0, 0, 0], "1e12 collapses to the corner"
    assert geo[20][1][0] == -2 ** 31 and geo[20][1][2] == -2 ** 31, "NaN width"
    assert geo[21][0][0] > geo[21][0][2], "x0 > x1"
    assert tuple(m["out"][0, 0]) == (255, 128, 30) and tuple(m["out"][1, 0]) == (255, 128, 30), "the 1e12 record: corner (0, 0), tag from row 1"
    assert tuple(m["out"][30, 0]) == (128, 30, 255), "the NaN-width record: a box at column 0"
    # the text: black on bright tags, white on dark ones
    txt = {tuple(int(v) for v in p) for p in m["out"].reshape(-1, 3)}
    assert (0, 0, 0) in txt and (255, 255, 255) in txt
    for name, c in cases.items():
        assert (c["out"] != c["frame"]).any() == (c["drawn"] > 0), name

    BG = 7     # no palette or text colour has this byte

    def on(img):
        return (img != BG).any(axis=2)

    def solo(i):
        """record i of the main case painted alone on a plain frame, by the reference (lib is still loaded)"""
        return ref_draw(lib, np.full_like(m["frame"], BG), m["cls"][i:i + 1], m["box"][i:i + 1], .1, m["labels"])[0]

    # overlaps: the reference painting a pair leaves the later record's pixels wherever both paint, and they differ there
    for first, second in ((7, 8), (9, 10)):
        a, b = solo(first), solo(second)
        pair = ref_draw(lib, np.full_like(m["frame"], BG), m["cls"][first:second + 1], m["box"][first:second + 1], .1, m["labels"])[0]
        both = on(a) & on(b)
        assert both.any() and (a[both] != b[both]).any() and (pair == np.where(on(b)[:, :, None], b, a)).all(), "the later record of a pair wins"
    # the tag of record 6 runs off the right edge: its background reaches the last column
    assert on(solo(6))[:, 95].any()
    # %.2f ties and carry: the texts are those of 0.12, 0.38 and 1.00 (the same record with that prob)
    for i, text_prob in ((14, .12), (15, .38), (16, 1.)):
        twin = m["box"][i:i + 1].copy()
        twin[0, 0] = text_prob
        assert (solo(i) == ref_draw(lib, np.full_like(m["frame"], BG), m["cls"][i:i + 1], twin, .1, m["labels"])[0]).all(), text_prob
    # labels = NULL gives "class3": the same pixels as a label list that says so
    nl = cases["nolabels"]
    assert (nl["out"] == ref_draw(lib, nl["frame"], nl["cls"], nl["box"], .1, ["a", "b", "c", "class3"])[0]).all()
    # the long label is cut at 127 characters: on a frame wide enough for it the tag is exactly that wide
    lc = cases["longlabel"]
    cols = np.nonzero(on(ref_draw(lib, np.full((24, 1800, 3), BG, dtype=np.uint8), lc["cls"], lc["box"], .1, lc["labels"])[0]).any(axis=0))[0]
    assert cols.max() - cols.min() == (127 * 6 - 1) * 2 + 4, "a tag of exactly 127 characters"

    out = {"cases": np.array(list(cases)), "font/chars": np.array(FONT_CHARS), "font/bitmaps": bitmaps, "font/words": words}
    for name, c in cases.items():
        out[name + "/frame"] = c["frame"]
        out[name + "/cls"] = c["cls"]
        out[name + "/box"] = c["box"]
        out[name + "/thresh"] = c["thresh"]
        out[name + "/n_labels"] = np.int32(-1 if c["labels"] is None else len(c["labels"]))   # -1: labels = NULL
        out[name + "/labels"] = np.array(c["labels"] if c["labels"] else [""])
        painted = (c["out"] != c["frame"]).any(axis=2)
        out[name + "/painted"] = painted                               # where the output differs from the frame ...
        out[name + "/paint"] = c["out"] * painted[:, :, None]          # ... and its pixels there (0 elsewhere)
        out[name + "/drawn"] = np.int32(c["drawn"])
    path = os.path.join(HERE, "draw.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 150 * 1024, size
    print(f"wrote {path}: {size} bytes, {len(cases)} cases")
    print("font words:", ", ".join(f"0x{int(v):09x}" for v in words))


if __name__ == "__main__":
    main()
