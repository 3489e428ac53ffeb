"""Option jpegdec_split without a GPU: the entropy stage with many lanes per restart interval (csrc/jpeg_scan.hpp: SBits, split_run;
csrc/jpeg_parse.hpp: split_plan, split_segment_host), run on the host through yolo2_hip_decode_jpeg_split_ref with the lanes and
rounds as loops.  The bar is exactness: the bytes of the host decoder on intact streams, and on every stream the status and bytes of
the one-lane doorway yolo2_hip_decode_jpeg_ref (tests/test_jpegdec_host.py has held that one against the host decoder)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpegdec_cases as jc
from jpegsplit_cases import noise_streams
import orclib
from yolo2_amd import hipdrv

ACCEPTED = [n for n in jc.JPEGS if hipdrv.jpeg_probe(jc.stream(n))["gpu_decodable"]]


def _longest_segment(data: bytes) -> int:
    """bytes of the longest stretch of entropy-coded data between two markers of the scan"""
    scan = jc.header_facts(data)["scan"]
    cuts = [scan] + [p + 2 for p in jc.rst_positions(data, scan)] + [len(data)]
    return max(b - a for a, b in zip(cuts, cuts[1:])) - 4        # (less the markers at its end; a lower bound is what the test needs)


@pytest.mark.parametrize("split", [32, 64, 128, 1024])
def test_fixtures_decode_to_the_host_decoders_bytes_without_falling_back(split):
    assert len(ACCEPTED) == 20
    for name in ACCEPTED:
        data = jc.stream(name)
        got, status, info = hipdrv.jpeg_decode_ref(data, split=split)
        want = jc.host_decode_fixture(name)
        assert status == 0 and got.shape == want.shape and np.array_equal(got, want), (name, split, status)
        assert info["split_bytes"] == split and info["fallback_segments"] == 0, (name, info)
        if _longest_segment(data) > 2 * split:
            assert info["split_segments"] >= 1, (name, info)
        assert info["max_rounds"] <= max(0, info["subsequences"] - 1), (name, info)
        if info["split_segments"]:
            assert info["subsequences"] >= 2 * info["split_segments"] and info["max_rounds"] >= 1, (name, info)


def test_rounds_stay_within_a_segments_subsequences():
    """one segment: the round count is bounded by ITS subsequences less one (the only cap of the algorithm)"""
    for name in ("jpg/base_444", "jpg/base_420_q100", "jpg/grey", "ref/cat.jpg"):
        assert jc.header_facts(jc.stream(name))["dri"] == 0
        for split in (32, 128):
            _, status, info = hipdrv.jpeg_decode_ref(jc.stream(name), split=split)
            assert status == 0 and info["split_segments"] == 1 and 1 <= info["max_rounds"] <= info["subsequences"] - 1, (name, info)
            assert info["subsequences"] <= 2048                              # the subsequence is doubled until they fit


@pytest.mark.parametrize("split", [32, 128])
def test_damaged_streams_give_the_one_lane_doorways_status_and_bytes(split):
    fell_back = []
    seen = set()
    for label, data in sorted(jc.damaged().items()):
        want, want_status = hipdrv.jpeg_decode_ref(data)
        got, status, info = hipdrv.jpeg_decode_ref(data, split=split)
        assert status == want_status, (label, status, want_status)
        assert (got is None) == (want is None) and (got is None or np.array_equal(got, want)), label
        seen.add(status if status < 100 else 100)
        if info["fallback_segments"] and label.endswith((":stray_eoi", ":truncated")):
            fell_back.append(label)
    assert fell_back, "no stray_eoi / truncated copy reached the fallback"
    assert {0, 3, 100} <= seen                                               # decoded, flagged and refused copies were all among them


@pytest.mark.parametrize("split", [32, 128])
def test_noise_streams_and_the_slow_synchroniser(split):
    """long codes, no DRI; the small ones are too short to split"""
    short = split_count = 0
    for data in list(noise_streams()) + [jc.stream("jpg/base_420_q100")]:
        want, want_status = hipdrv.jpeg_decode_ref(data)
        got, status, info = hipdrv.jpeg_decode_ref(data, split=split)
        assert status == want_status == 0 and np.array_equal(got, want) and np.array_equal(got, jc.host_decode(data))
        assert info["fallback_segments"] == 0
        short += info["short_segments"]
        split_count += info["split_segments"]
    assert short >= 2 and split_count >= 3
    _, _, info = hipdrv.jpeg_decode_ref(jc.stream("jpg/base_420_q100"), split=32)
    assert info["max_rounds"] > 100                                          # it barely synchronises, and is exact all the same


def test_option_is_named_documented_and_range_checked():
    src = open(os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd", "csrc", "yolo2_plan.hip")).read()
    assert '{"jpegdec_split", &Y2Options::jpegdec_split, 16, 4096}' in src
    readme = open(os.path.join(orclib.ROOT, "README.md")).read()
    assert "`jpegdec_split`" in readme
    L = hipdrv.lib()
    so = lambda v: L.yolo2_hip_set_option(None, b"jpegdec_split", v)
    try:
        for ok in (b"16", b"128", b"4096", b"0"):
            assert so(ok) == hipdrv.YOLO2_SUCCESS, ok
        for bad in (b"8", b"100", b"4112", b"-16", b"x"):
            assert so(bad) == hipdrv.YOLO2_ERROR and b"out of range" in L.yolo2_hip_last_error(), bad
    finally:
        assert so(None) == hipdrv.YOLO2_SUCCESS
    # the doorway checks the same range
    data = jc.stream("jpg/base_420")
    for bad in (0, 8, 100, 4112):
        with pytest.raises(hipdrv.Yolo2HipError, match="multiple of 16"):
            hipdrv.jpeg_decode_ref(data, split=bad)
    assert {"yolo2_hip_decode_jpeg_split_ref", "yolo2_hip_jpeg_split_info"} <= set(hipdrv.EXPORTS)


def test_split_and_one_lane_agree_on_mutated_streams_under_sanitizers(tmp_path):
    """tools/fuzz_jpegdec_split.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer: the split doorway against decode_ref over
    the fixture streams and mutated copies (bit flips, truncations, runs of 0xff) at two subsequence sizes.  A stand-alone program;
    nothing is loaded into this process."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    pkg = os.path.join(orclib.ROOT, "yolo-fpga-accelerator_amd")
    exe = tmp_path / "fuzz_jpegdec_split"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", str(exe), os.path.join(pkg, "tools", "fuzz_jpegdec_split.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    files = []
    for name in jc.JPEGS:
        if name in ("ref/image2.jpg", "ref/image1.jpg", "ref/desk.jpg", "ref/timg.jpg", "ref/cat.jpg", "ref/dog.jpg", "ref/person.jpg"):
            continue                                # large: time (the first test has them intact)
        f = tmp_path / name.replace("/", "_")
        f.write_bytes(jc.stream(name))
        files.append(str(f))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1:hard_rss_limit_mb=4000")
    run = subprocess.run([str(exe), "60", "32", "128"] + files, capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    same, split, fallbacks, refused, mismatch = [int(x) for x in run.stdout.replace(",", "").split() if x.isdigit()]
    assert mismatch == 0
    assert same > 1000 and split > 0 and fallbacks > 0 and refused > 0       # both routes and the refusals were all reached
