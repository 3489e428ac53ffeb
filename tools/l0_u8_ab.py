#!/usr/bin/env python3
"""Layer-0 A/B of the images entries (GPU box): the fused k_conv0_pool_mfma_u8 (layers 0+1 from image bytes) against the two-kernel
route it replaces - k_letterbox_u8_batch (as the int16 images entry launches it) + k_conv0_pool_mfma on the letterboxed frames - on the
same images, fp16 at batch 256 and split-fp16 at batch 128 (two lanes each).  Run it under rocprofv3, then summarize:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ab -- python3 tools/l0_u8_ab.py <h> <w>
  python3 tools/l0_u8_ab.py --summary <dir>/ab_kernel_stats.csv <h> <w>"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-fpga-accelerator_amd"))
REPS = 16
PASSES = ((256, False), (128, True))


def summary(csv_path, h, w):
    import csv
    rows = {r["Name"]: r for r in csv.DictReader(open(csv_path))}
    def stat(prefix):   # (launches, ms) of the kernel whose (mangled or demangled) name starts with prefix
        hits = [r for n, r in rows.items() if n.startswith(prefix)]
        assert len(hits) == 1, (prefix, list(rows))
        return int(hits[0]["Calls"]), float(hits[0]["TotalDurationNs"]) / 1e6
    lb_calls, lb_ms = stat("y2::k_letterbox_u8_batch")
    lb_frames = REPS * sum(B for B, _ in PASSES)      # one launch per chunk, every pass at its own batch
    print(f"# layer-0 A/B, {w}x{h} RGB images, {REPS} calls per form and pass: rocprofv3 --kernel-trace --stats, summed kernel time per frame")
    print(f"k_letterbox_u8_batch   {lb_calls:3d} launches {lb_ms:8.3f} ms  {lb_ms * 1e3 / lb_frames:6.2f} us/frame (fp16 and split chunks)")
    for B, split in PASSES:
        tag = "1" if split else "0"
        nf = REPS * B
        fu_c, fu_ms = stat(f"_ZN2y220k_conv0_pool_mfma_u8ILb{tag}E")
        fr_c, fr_ms = stat(f"_ZN2y217k_conv0_pool_mfmaILb{tag}E")
        two = lb_ms * 1e3 / lb_frames + fr_ms * 1e3 / nf
        print(f"{'split' if split else 'fp16 '} batch {B}: k_conv0_pool_mfma_u8 {fu_c} launches {fu_ms:7.3f} ms = {fu_ms * 1e3 / nf:5.2f} us/frame | "
              f"k_conv0_pool_mfma {fr_c} launches {fr_ms:7.3f} ms = {fr_ms * 1e3 / nf:5.2f} us/frame, + letterbox = {two:5.2f} us/frame | "
              f"fused / two-kernel = {fu_ms * 1e3 / nf / two:.3f}")


def run(h, w):
    import numpy as np
    import torch
    from yolo2_amd import hipdrv, synth
    rng = np.random.default_rng(5)
    model = synth.SynthModel(seed=1)
    ctx = hipdrv.Yolo2Hip(0)
    ctx.load_model(model)
    ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
    base = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(16)]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for B, split in PASSES:
        imgs = [base[i % 16] for i in range(B)]
        for _ in range(REPS):
            ctx.run_images_f16_host(imgs, B, split=split)                 # fused
        for _ in range(REPS):
            ctx.run_images_host(imgs, batch=B)                            # k_letterbox_u8_batch at the same batch
        frames = torch.from_numpy(np.stack([hipdrv.letterbox_u8(im) for im in base] * (B // 16))).to(dev)
        region = torch.empty((B, 425, 13, 13), dtype=torch.float32, device=dev)
        fn = ctx.run_batch_f32tol_ptr if split else ctx.run_batch_fp16_ptr
        for _ in range(REPS):
            fn(frames.data_ptr(), B, region.data_ptr(), st)               # k_conv0_pool_mfma on the letterboxed frames
        torch.cuda.synchronize()
        print(f"batch {B} {'split' if split else 'fp16'}: images layer 0 = {ctx.images_layer0_kernel(split)}")
    ctx.close()


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        run(int(sys.argv[1]), int(sys.argv[2]))
