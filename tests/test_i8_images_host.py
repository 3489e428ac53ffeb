"""The int8 images entries, the parts that need no GPU: the three names are declared, exported and bound; hipdrv accepts the
precision and refuses the multi-GPU form before any library call; the option of the reference route is named and documented."""
import ctypes
import os
import re

import numpy as np
import pytest

import orclib
from yolo2_amd import hipdrv

ROOT = orclib.ROOT
NAMES = ("yolo2_hip_run_images_pix_int8_host", "yolo2_hip_run_images_pix_dets_int8", "yolo2_hip_images_front_kernel_int8")


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "yolo2_hip.h")).read()
    L = ctypes.CDLL(hipdrv.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(yolo2_hip_ctx \*ctx", header), name
        assert hasattr(L, name), name
        assert name in hipdrv.EXPORTS, name
    assert "have no int8 form. */" not in header.replace("The loop and multi-GPU entries have no int8 form. */", "")


def test_hipdrv_takes_the_precision_and_refuses_the_multi_form_before_any_call(monkeypatch):
    assert "int8" in hipdrv.PRECISIONS
    assert hipdrv.LOOP_PRECISIONS == {"int16": 0, "fp16": 1, "fp32fast": 2}       # the loop entries have no int8 form
    monkeypatch.setattr(hipdrv, "lib", lambda: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="int8"):
        hipdrv.run_images_dets(None, [np.zeros((4, 4, 3), np.uint8)], 1, 0.1, 0.45, precision="int8", multi=True)
    assert hasattr(hipdrv.Yolo2Hip, "run_images_int8_host") and hasattr(hipdrv.Yolo2Hip, "images_front_kernel_int8")


def test_option_of_the_reference_route_is_named_and_documented():
    src = open(os.path.join(ROOT, "yolo-fpga-accelerator_amd", "csrc", "yolo2_plan.hip")).read()
    assert '{"i8_no_front", &Y2Options::i8_no_front}' in src
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`i8_no_front`" in readme
    L = hipdrv.lib()
    assert L.yolo2_hip_set_option(None, b"i8_no_front", b"1") == hipdrv.YOLO2_SUCCESS
    assert L.yolo2_hip_set_option(None, b"i8_no_front", None) == hipdrv.YOLO2_SUCCESS
