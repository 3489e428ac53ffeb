#!/usr/bin/env python3
"""Layer-0 A/B of the YUYV camera format (GPU box): k_conv0_pool_mfma_yuyv (layers 0+1 from packed YUYV 4:2:2 bytes, converted per
fetched pixel) against k_conv0_pool_mfma_u8 on the same frames converted to RGB24, fp16 at batch 256 and split-fp16 at batch 128 (two
lanes each), the two forms alternating.  Run it under rocprofv3 (no counters), then summarize:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ab -- python3 tools/l0_yuyv_ab.py <h> <w>
  python3 tools/l0_yuyv_ab.py --summary <dir>/ab_kernel_stats.csv <h> <w>"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS = 16
PASSES = ((256, False), (128, True))


def summary(csv_path, h, w):
    import csv
    rows = {r["Name"]: r for r in csv.DictReader(open(csv_path))}
    def stat(prefix):   # the kernel whose mangled name starts with prefix: launches, us per frame (mean, fastest and slowest launch)
        hits = [r for n, r in rows.items() if n.startswith(prefix)]
        assert len(hits) == 1, (prefix, list(rows))
        r = hits[0]
        return int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3
    print(f"# layer-0 A/B, {w}x{h} frames, {REPS} calls per form and pass, alternating: rocprofv3 --kernel-trace --stats, summed kernel time per frame "
          f"(fastest .. slowest launch)")
    for B, split in PASSES:
        tag = "1" if split else "0"
        out = []
        for name, prefix in (("k_conv0_pool_mfma_yuyv", f"_ZN2y222k_conv0_pool_mfma_yuyvILb{tag}E"), ("k_conv0_pool_mfma_u8", f"_ZN2y220k_conv0_pool_mfma_u8ILb{tag}E")):
            calls, total, lo, hi = stat(prefix)
            per_launch = REPS * B / calls          # frames of one launch (a lane's share of the chunk)
            out.append(total / (REPS * B))
            print(f"{'split' if split else 'fp16 '} batch {B}: {name:23s} {calls:3d} launches {total / 1e3:8.3f} ms = {total / (REPS * B):5.2f} us/frame "
                  f"({lo / per_launch:5.2f} .. {hi / per_launch:5.2f})")
        print(f"{'split' if split else 'fp16 '} batch {B}: yuyv / u8 = {out[0] / out[1]:.3f}")


def run(h, w):
    import numpy as np
    from yolo2_amd import hipdrv, synth
    from yuyvref import formula
    rng = np.random.default_rng(5)
    model = synth.SynthModel(seed=1)
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    base = [rng.integers(0, 256, (h, w, 2), dtype=np.uint8) for _ in range(16)]
    conv = [formula(f) for f in base]
    for B, split in PASSES:
        yuyv, rgb = [base[i % 16] for i in range(B)], [conv[i % 16] for i in range(B)]
        for _ in range(REPS):
            a = ctx.run_images_f16_host(yuyv, B, split=split, pixfmt="yuyv")
            ka = ctx.images_layer0_kernel(split)
            b = ctx.run_images_f16_host(rgb, B, split=split)
            kb = ctx.images_layer0_kernel(split)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        print(f"batch {B} {'split' if split else 'fp16'}: {ka} against {kb}: same bits")
    ctx.close()


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        run(int(sys.argv[1]), int(sys.argv[2]))
