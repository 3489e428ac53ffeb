"""The GPU JPEG decoder's host side, without a GPU: the probe (yolo2_hip_jpeg_probe) and the host doorway (yolo2_hip_decode_jpeg_ref),
which runs the very functions of csrc/jpeg_scan.hpp that the kernels run.  Expected side: the fixtures of tests/golden/images.npz and the
host decoder y2h_decode_image (pinned to stb_image by tests/test_host_codec.py), never the code under test.

The fixture file holds 30 JPEG streams: 20 baseline ones of 1 or 3 components (all seven of the reference's own ref/*.jpg with content
among them, three with DRI 80, 96 and 169), 9 progressive ones and jpg/cmyk.  The expected class of each comes from a header reader of
this test's own (jpegdec_cases.header_facts)."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import orclib
import jpegdec_cases as jc
from yolo2_amd import hipdrv

REASON = {name: k for k, name in enumerate(hipdrv.JPEG_REASONS)}


def _expected_class(data: bytes):
    f = jc.header_facts(data)
    if f["sof"] == 0xC2:
        return "progressive"
    if f["ncomp"] == 4:
        return "components"
    assert f["sof"] in (0xC0, 0xC1) and f["ncomp"] in (1, 3)
    return "accepted"


def test_probe_classifies_the_fixture_streams():
    accepted, refused = [], {}
    for name in jc.JPEGS:
        data = jc.stream(name)
        info = hipdrv.jpeg_probe(data)
        want = _expected_class(data)
        assert hipdrv.JPEG_REASONS[info["reason"]] == want, (name, info)
        assert info["gpu_decodable"] == int(want == "accepted"), name
        assert info["stream_bytes"] == len(data), (name, info)         # every fixture ends with its EOI
        if want == "accepted":
            f = jc.header_facts(data)
            assert (info["width"], info["height"], info["components"], info["restart_interval"]) == (f["width"], f["height"], f["ncomp"], f["dri"]), name
            assert (info["height"], info["width"]) == tuple(jc.IMAGES[f"{name}/shape"])[:2], name
            accepted.append(name)
        else:
            refused[name] = want
    ref = [n for n in accepted if n.startswith("ref/")]
    assert len(ref) == 7, ref                                            # all of the reference's own files with content
    assert sorted(hipdrv.jpeg_probe(jc.stream(n))["restart_interval"] for n in ref)[-3:] == [80, 96, 169]
    assert "jpg/restart_blocks" in accepted and "jpg/restart_rows" in accepted and "jpg/grey" in accepted
    assert refused["jpg/cmyk"] == "components"
    assert sorted(refused.values()).count("progressive") == len(refused) - 1 and len(refused) >= 8
    assert len(accepted) + len(refused) == len(jc.JPEGS) and len(accepted) >= 20


@pytest.mark.parametrize("mangle,reason", [
    (lambda d: b"\x00" + d[1:], "damaged"),                                   # no SOI
    (lambda d: d[:40], "damaged"),                                            # cut inside the headers
    (lambda d: d[:-2], "damaged"),                                            # no EOI
    (lambda d: d[:-2] + b"\xff\xc4\x00\x02\xff\xd9", "scans"),                 # a segment between the scan and EOI
    (lambda d: d.replace(b"\xff\xc0", b"\xff\xc9", 1), "unsupported_sof"),    # arithmetic coding
])
def test_probe_refuses_what_it_cannot_vouch_for(mangle, reason):
    info = hipdrv.jpeg_probe(mangle(jc.stream("jpg/base_420")))
    assert not info["gpu_decodable"] and hipdrv.JPEG_REASONS[info["reason"]] == reason, info


def _with_sof_bytes(data: bytes, patch):
    d = bytearray(data)
    i = 2
    while d[i + 1] not in (0xC0, 0xC1):
        i += 2 + ((d[i + 2] << 8) | d[i + 3])
    patch(d, i)
    return bytes(d)


def test_probe_refuses_sampling_colour_and_missing_tables():
    base = jc.stream("jpg/base_420")
    def factors(hv):
        def patch(d, i):
            for k, (h, v) in enumerate(hv):
                d[i + 10 + 3 * k + 1] = (h << 4) | v
        return patch
    for hv in ([(4, 1), (1, 1), (1, 1)], [(2, 2), (2, 1), (1, 1)], [(4, 4), (1, 1), (1, 1)]):
        info = hipdrv.jpeg_probe(_with_sof_bytes(base, factors(hv)))
        assert hipdrv.JPEG_REASONS[info["reason"]] == "sampling", (hv, info)
    def rgb_ids(d, i):
        for k, c in enumerate(b"RGB"):
            d[i + 10 + 3 * k] = c
    # the scan header names the components by id too: patch both
    d = bytearray(_with_sof_bytes(base, rgb_ids))
    sos = d.index(b"\xff\xda")
    for k, c in enumerate(b"RGB"):
        d[sos + 5 + 2 * k] = c
    assert hipdrv.JPEG_REASONS[hipdrv.jpeg_probe(bytes(d))["reason"]] == "rgb_colour"
    d = bytearray(base)
    sos = d.index(b"\xff\xda")
    d[sos + 6] = 0x33                    # component 1 names DC / AC tables 3, which no DHT defines
    assert hipdrv.JPEG_REASONS[hipdrv.jpeg_probe(bytes(d))["reason"]] == "missing_table"


@pytest.mark.parametrize("junk", [b"", b"\x00\x01junk between frames\x02", b"\xff\xff\x00\xff"])
def test_probe_cuts_a_concatenated_stream(junk):
    names = ["jpg/restart_rows", "ref/person.jpg", "jpg/prog_420"]      # DRI, DRI + h1v2, progressive (several scans)
    parts = [jc.stream(n) for n in names]
    buf = junk.join(parts) + junk
    at, cut = 0, []
    while True:
        at = buf.find(b"\xff\xd8", at)
        if at < 0:
            break
        n = hipdrv.jpeg_probe(buf[at:])["stream_bytes"]
        cut.append(buf[at:at + n])
        at += n
    assert cut == parts


@pytest.mark.parametrize("name", [n for n in jc.JPEGS if _expected_class(jc.stream(n)) == "accepted"])
def test_doorway_equals_the_host_decoder_and_the_fixture(name):
    got, status = hipdrv.jpeg_decode_ref(jc.stream(name))
    assert status == 0
    want = jc.host_decode_fixture(name)
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"
    if f"{name}/rgb" in jc.IMAGES:
        assert np.array_equal(got, jc.IMAGES[f"{name}/rgb"]), name
    else:
        assert np.array_equal(got[::41], jc.IMAGES[f"{name}/rgb_rows"]), name
    assert hashlib.sha256(got.tobytes()).digest() == jc.IMAGES[f"{name}/sha256"].tobytes(), name


def test_doorway_refuses_a_short_buffer_and_reports_refused_streams():
    got, status = hipdrv.jpeg_decode_ref(jc.stream("jpg/prog_420"))
    assert got is None and status == 100 + REASON["progressive"]
    with pytest.raises(hipdrv.Yolo2HipError, match="too small"):
        hipdrv.jpeg_decode_ref(jc.stream("jpg/base_420"), cap=97 * 61 * 3 - 1)


@pytest.mark.parametrize("label", sorted(jc.damaged()))
def test_damaged_scans_are_flagged_or_decoded_as_the_host_decodes_them(label):
    """status 0 with the host decoder's bytes, or a non-zero status (100 + reason: refused by the probe); never status 0 with other
    bytes; non-zero wherever the host decoder throws"""
    data = jc.damaged()[label]
    got, status = hipdrv.jpeg_decode_ref(data)
    want = jc.host_decode(data)
    if want is None:
        assert status != 0, label
    if status == 0:
        assert want is not None and got.shape == want.shape and np.array_equal(got, want), label
    else:
        assert got is None


def test_damage_list_reaches_every_status_class():
    """the list above is not all refusals: some damaged copies decode (status 0), some are flagged by the scan (1..3), some refused"""
    st = {label: hipdrv.jpeg_decode_ref(d)[1] for label, d in jc.damaged().items()}
    assert any(s == 0 for s in st.values()) and any(0 < s < 100 for s in st.values()) and any(s >= 100 for s in st.values()), st
    assert st["jpg/restart_rows:rst_removed"] == 3 and st["jpg/restart_blocks:rst_duplicated"] == 3, st


def test_decoder_stages_survive_damaged_streams_under_sanitizers(tmp_path):
    """tools/fuzz_jpegdec.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer: the doorway over every fixture stream and 200
    mutated copies of each.  A stand-alone program; nothing is loaded into this process."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    pkg = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")
    exe = tmp_path / "fuzz_jpegdec"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", str(exe), os.path.join(pkg, "tools", "fuzz_jpegdec.cpp"), os.path.join(pkg, "host", "y2_codec.cpp"),
                         os.path.join(pkg, "host", "y2_host.cpp"), "-pthread"], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    files = []
    for name in jc.JPEGS:
        if name in ("ref/image2.jpg", "ref/image1.jpg", "ref/desk.jpg", "ref/timg.jpg", "ref/cat.jpg"):
            continue                                # large and without a restart interval or sampling of their own: time
        f = tmp_path / name.replace("/", "_")
        f.write_bytes(jc.stream(name))
        files.append(str(f))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1:hard_rss_limit_mb=4000")
    run = subprocess.run([str(exe), "200"] + files, capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    same, flagged, refused, wrong = [int(x) for x in run.stdout.replace(",", "").split() if x.isdigit()]
    assert wrong == 0
    assert same >= len([n for n in files]) - 10 and flagged > 0 and refused > 0     # undamaged accepted files decode; damage is noticed both ways
