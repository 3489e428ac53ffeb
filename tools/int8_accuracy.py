#!/usr/bin/env python3
"""Accuracy of the int8 pass's DEFINITION (tests/i8ref.py) against the float pass in float64 on the same weights, with the int16 pass
(the oracle's restatement of the reference, SynthModel's hand-picked Q tables) beside it.  CPU only.  SynthModel(seed=1), calibrated
on synth.frames(40, 4), evaluated on synth.frames(41, 2): the setup tests/test_i8_host.py asserts on.
Writes profiles/r13_int8_accuracy.txt.  usage: python3 tools/int8_accuracy.py [out]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import i8ref, orclib
from yolo2_amd import synth

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_int8_accuracy.txt")
model = synth.SynthModel(seed=1)
w, b = i8ref.model_f32(model)
_, absmax = i8ref.float_forward(synth.frames(40, 4), w, b)
act_q = i8ref.act_q_from_stats(absmax, 1.0)
m = i8ref.ModelI8(w, b, act_q)
ev = synth.frames(41, 2)
want, _ = i8ref.float_forward(ev, w, b)


def figures(got):
    d = got.astype(np.float64) - want
    return float(np.sqrt(np.mean(d ** 2))), float(np.abs(d).max()), i8ref.mean_iou(got, want)


orclib.oracle().orc_set_threads(min(16, os.cpu_count() or 1))
r16 = np.stack([orclib.forward_i16(model, f)[1].reshape(425, 13, 13) for f in ev])
rows = [("int8 (tests/i8ref.py)", figures(i8ref.forward(ev, m))), ("int16 (oracle, Q tables of SynthModel)", figures(r16))]
qw = np.concatenate(m.qw)
lines = ["int8 definition against the float pass (float64, same weights): SynthModel(seed=1), calibrated on synth.frames(40, 4),",
         "evaluated on synth.frames(41, 2); region tensor std %.3f" % want.std(), "",
         "activation Qs: %s" % " ".join(str(int(q)) for q in act_q), "weight Qs per channel: %d..%d" % (qw.min(), qw.max()), "",
         "%-42s %-12s %-12s %s" % ("pass", "rms error", "max error", "mean box IoU over all 845 slots")]
for name, (rms, mx, iou) in rows:
    lines.append("%-42s %-12.5f %-12.5f %.4f" % (name, rms, mx, iou))
lines += ["", "fp16 pass: no CPU restatement of the whole pass exists in the fixtures (tests/f16ref.py judges it launch by launch on the GPU);",
          "README quotes its boxes within IoU 0.97 (mean 0.9975) of the fp32 oracle's.",
          "tests/test_i8_host.py asserts rms <= 0.14 and mean IoU >= 0.75 on the int8 row."]
text = "\n".join(lines) + "\n"
print(text)
open(out_path, "w").write(text)
