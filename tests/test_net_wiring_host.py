"""The library's wiring table (csrc/y2_internal.hpp NetWire, built in csrc/yolo2_hip.hip) against an independent derivation: the
[route] sections of the two cfg files, parsed here, plus yolo2_amd/net.py's layer table and stream lengths.  And the hole the table
closes: a cfg whose routes name other layers is refused by yolov2_detect before any device is touched.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

from yolo2_amd import hipdrv, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = [os.path.join(hipdrv.PKG_DIR, "config", "yolov2.cfg"), os.path.join(ROOT, "tests", "golden", "ref_yolov2.cfg")]
DETECT = os.path.join(hipdrv.PKG_DIR, "yolov2_detect")


def cfg_routes(path):
    """{route layer: [absolute source layers, in the cfg's order]}; a negative index is relative to the route layer."""
    sections = re.findall(r"^\[(\w+)\]([^\[]*)", open(path).read(), flags=re.M)
    assert sections[0][0] == "net"
    routes = {}
    for idx, (name, body) in enumerate(sections[1:]):
        if name == "route":
            listed = re.search(r"^layers\s*=\s*(.+)$", body, flags=re.M).group(1)
            routes[idx] = [int(v) + idx if int(v) < 0 else int(v) for v in listed.split(",")]
    return len(sections) - 1, routes


def derive(routes):
    """per layer: ord, w_off, b_off, src, cat, ch_off, readers, reader, to_region, C, H, W - from net.LAYERS and the routes alone"""
    L = net.LAYERS
    own = [(l.out_c, l.out_h, l.out_w) for l in L]

    def tensor_of(i):                       # the layer whose tensor stands for layer i's output
        if L[i].type != net.ROUTE:
            return i
        return tensor_of(routes[i][0]) if len(routes[i]) == 1 else i

    place = {}                              # member -> (concat layer, first channel)
    shape = list(own)
    for r, srcs in routes.items():
        if len(srcs) == 1:
            shape[r] = own[tensor_of(r)]
            continue
        off = 0
        for m in srcs:
            place[m] = (r, off)
            off += own[m][0]
        assert len({own[m][1:] for m in srcs}) == 1
        shape[r] = (off,) + own[srcs[0]][1:]
        place[r] = (r, 0)
        for m in srcs:
            shape[m] = shape[r]
    src = [-1 if i == 0 else tensor_of(i - 1) for i in range(len(L))]
    for r in routes:
        src[r] = tensor_of(r)
    readers = [[] for _ in L]
    for i, l in enumerate(L):
        if l.type == net.ROUTE or src[i] < 0:
            continue
        for j in range(len(L)):
            if j == src[i] or (j in place and place[j][0] == src[i]):
                readers[j].append(i)
    rows, woff, boff = [], 0, 0
    for i, l in enumerate(L):
        conv = l.type == net.CONV
        rows.append([l.ord if conv else -1, woff if conv else 0, boff if conv else 0, src[i], place.get(i, (-1, 0))[0], place.get(i, (-1, 0))[1],
                     len(readers[i]), readers[i][0] if readers[i] else -1, int(any(L[k].type == net.REGION for k in readers[i])), *shape[i]])
        if conv:
            woff += net.WEIGHT_LEN[l.ord]
            boff += net.BIAS_LEN[l.ord]
    assert (woff, boff) == (net.N_WEIGHTS, net.N_BIAS)
    return rows


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(hipdrv.LIB_PATH)
    L.yolo2_hip_layer_routes.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.yolo2_hip_debug_layer_wiring.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return L


@pytest.mark.parametrize("cfg", CFGS, ids=["package", "reference"])
def test_wiring_table_equals_the_cfg(lib, cfg):
    n, routes = cfg_routes(cfg)
    assert n == len(net.LAYERS) == lib.yolo2_hip_num_layers() == 32
    assert routes == {25: [16], 28: [27, 24]}   # what both files say today, in their own words: layers=-9 and layers=-1,-4
    want = derive(routes)
    # the facts the passes used to spell out by hand
    assert want[26][3] == 16 and want[29][3] == 28 and want[24][4:6] == [28, 256] and want[27][4:6] == [28, 0] and want[16][6] == 2
    assert [i for i in range(32) if want[i][8]] == [30] and want[28][9:] == [1280, 13, 13]
    for i in range(32):
        src, out = (ctypes.c_int * 4)(), (ctypes.c_int * 12)()
        k = lib.yolo2_hip_layer_routes(i, src)
        assert list(src)[:max(k, 0)] == routes.get(i, []) and k == len(routes.get(i, [])), f"layer {i}: routes {list(src)[:k]}"
        assert lib.yolo2_hip_debug_layer_wiring(i, out) == 0
        assert list(out) == want[i], f"layer {i}: library {list(out)}, cfg {want[i]}"
    assert lib.yolo2_hip_layer_routes(32, src) == hipdrv.YOLO2_ERROR and lib.yolo2_hip_layer_routes(-1, src) == hipdrv.YOLO2_ERROR
    assert lib.yolo2_hip_layer_routes(0, None) == hipdrv.YOLO2_ERROR and lib.yolo2_hip_debug_layer_wiring(32, out) == hipdrv.YOLO2_ERROR


@pytest.mark.parametrize("streaming", [False, True], ids=["image", "stream"])
@pytest.mark.parametrize("first_route", ["-8", "-11"])
def test_detect_refuses_a_cfg_with_other_routes(tmp_path, first_route, streaming):
    """layers=-8 reads layer 17 (another shape: the conv behind it used to be refused instead, as layer 26); layers=-11 reads layer 14,
    which has layer 16's shape - every per-layer field agrees and the run used to be ACCEPTED, on the hard-wired topology."""
    text = open(CFGS[0]).read()
    assert text.count("layers=-9\n") == 1
    bad = tmp_path / "bad.cfg"
    bad.write_text(text.replace("layers=-9\n", f"layers={first_route}\n"))
    (tmp_path / "weights").mkdir()
    (tmp_path / "frames").mkdir()
    source = ["--input-dir", str(tmp_path / "frames")] if streaming else ["--input", str(tmp_path / "none.ppm")]
    r = subprocess.run([DETECT, "--backend", "hip", "--cfg", str(bad), "--names", os.path.join(hipdrv.PKG_DIR, "config", "coco.names"),
                        "--weights", str(tmp_path / "weights"), "--output", str(tmp_path / "out" / "x")] + source,
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "cfg layer 25 differs" in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-400:])
