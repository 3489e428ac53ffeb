"""tests/streamref.py's table of stream-taking entries against include/yolo2_hip.h itself (no GPU): an entry that gains a
`void *stream` cannot stay out of tests/test_gpu_streams.py, and what the table says of each entry - it enqueues and returns, or it
synchronises the stream - is what the header's words say."""
import os
import re

import streamref as sr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yolo2_hip.h")
PROTO = re.compile(r"\bint\s+(yolo2_hip_\w+)\s*\(([^;{}]*)\)\s*;")
COMMENT = re.compile(r"/\*.*?\*/", re.S)


def stream_entries():
    """{name: the comment block in front of the prototype (prototypes that follow one another share it)} for every prototype whose
    last parameter is `void *stream`"""
    text = open(HEADER).read()
    comments = [(m.end(), m.group(0)) for m in COMMENT.finditer(text)]
    code = COMMENT.sub(lambda m: " " * len(m.group(0)), text)          # (same offsets, no prototype look-alikes inside comments)
    out = {}
    for m in PROTO.finditer(code):
        params = [p.strip() for p in m.group(2).split(",")]
        if re.fullmatch(r"void\s*\*\s*stream", params[-1]):
            before = [c for end, c in comments if end <= m.start()]
            assert before, m.group(1)
            out[m.group(1)] = before[-1]
        else:
            # (a `const uint8_t *stream` is a JPEG byte stream, not a hipStream_t)
            assert not any(re.fullmatch(r"void\s*\*\s*\w*stream\w*", p) for p in params), f"{m.group(1)} takes a stream that is not its last parameter"
    return out


def test_the_table_holds_every_stream_taking_prototype_of_the_header():
    found = stream_entries()
    assert len(found) >= 15
    assert set(found) == set(sr.ENTRIES), sorted(set(found) ^ set(sr.ENTRIES))
    assert set(sr.ENTRIES.values()) == {"enqueue", "sync"}


def test_each_kind_is_what_the_header_says():
    for name, words in stream_entries().items():
        kind = "sync" if re.search(r"\bsynchronises\b", words) else "enqueue"
        assert sr.ENTRIES[name] == kind, f"{name}: the table says {sr.ENTRIES[name]}, the header's words say {kind}"
        if kind == "sync":
            assert "`stream`" in words, f"{name}: the words that say it synchronises do not name the stream"


def test_the_wrappers_pass_a_stream_through():
    """every hipdrv wrapper of a stream-taking entry has a `stream` argument that defaults to the null stream"""
    import inspect
    from yolo2_amd import hipdrv
    fns = [hipdrv.letterbox_u8, hipdrv.letterbox_pix, hipdrv.annotate_pix, hipdrv.jpeg_encode, hipdrv.absmax_f32, hipdrv.postprocess,
           hipdrv.Yolo2Hip.calib_frames, hipdrv.Yolo2Hip.run_batch_ptr, hipdrv.Yolo2Hip.run_batch_fp16_ptr, hipdrv.Yolo2Hip.run_batch_f32tol_ptr,
           hipdrv.Yolo2Hip.run_batch_fp32_ptr, hipdrv.Yolo2Hip.run_batch_int8_ptr]
    for f in fns:
        p = inspect.signature(f).parameters.get("stream")
        assert p is not None and p.default == 0, f.__qualname__
