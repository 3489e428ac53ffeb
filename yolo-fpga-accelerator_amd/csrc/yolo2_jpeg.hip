// yolo2_jpeg.hip -- RGB24 frames in device memory -> JPEG streams (include/yolo2_hip.h, "annotated frames as JPEG"): the stream the
// reference's MJPEG streamer sends for a frame, byte for byte, made by the eight launches of kernels_jpeg.hpp.  The host side here
// makes the tables (jpeg_tables.hpp), lays the work area out and enqueues; nothing is read back between the stages.  The batched
// entry that paints and encodes lives with the painter (yolo2_draw.hip) and comes through y2_jpeg.hpp.
#include "y2_internal.hpp"
#include "kernels_jpeg.hpp"
#include "y2_jpeg.hpp"

using namespace y2;

namespace {
size_t padded(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

size_t y2_jpeg_table_bytes(int nf) { return padded(sizeof(JpegHeader) + (size_t)nf * sizeof(JpegFrame)); }

// a frame the encoder takes: 1..65535 each way, and a bound below 2^31 bytes (the 32-bit offsets of stage D)
static bool jpeg_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && y2j::stream_bound(w, h) < ((size_t)1 << 31); }

extern "C" size_t yolo2_hip_jpeg_bound(int w, int h) { return jpeg_size_ok(w, h) ? y2j::stream_bound(w, h) : 0; }

int y2_jpeg_check_frame(int w, int h, int f)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return fail(YOLO2_ERROR, "jpeg: frame %d is %dx%d; width and height are 1..65535", f, w, h);
    if (!jpeg_size_ok(w, h)) return fail(YOLO2_ERROR, "jpeg: frame %d (%dx%d) is too large: its stream may take %zu bytes", f, w, h, y2j::stream_bound(w, h));
    return YOLO2_SUCCESS;
}

namespace {
// what one frame takes of the chunk's arrays; both the plan and the table add these up in frame order
struct FrameShare {
    int mcux, n_blk;
    unsigned n_wg, n_seg;
    size_t us_bytes;
};
FrameShare frame_share(int w, int h)
{
    FrameShare s;
    s.mcux = (w + 7) / 8;
    s.n_blk = 3 * s.mcux * ((h + 7) / 8);
    s.n_wg = (unsigned)((s.n_blk + kJpegBlocks - 1) / kJpegBlocks);
    s.us_bytes = padded(((size_t)s.n_blk * y2j::kBlockBitsMax + 7) / 8);
    s.n_seg = (unsigned)((s.us_bytes + kJpegSegBytes - 1) / kJpegSegBytes);
    return s;
}
}  // namespace

int y2_jpeg_plan(const Y2JpegFrameIn *frames, int nf, Y2JpegPlan *plan)
{
    Y2JpegPlan p;
    p.nf = nf;
    p.table_bytes = y2_jpeg_table_bytes(nf);
    size_t blocks = 0, groups = 0, us = 0, segs = 0;
    unsigned max_groups = 0, max_segs = 0;
    for (int f = 0; f < nf; ++f) {
        int rc;
        if ((rc = y2_jpeg_check_frame(frames[f].w, frames[f].h, f))) return rc;
        const FrameShare s = frame_share(frames[f].w, frames[f].h);
        blocks += (size_t)s.n_blk;
        groups += s.n_wg;
        us += s.us_bytes;
        segs += s.n_seg;
        max_groups = std::max(max_groups, s.n_wg);
        max_segs = std::max(max_segs, s.n_seg);
        p.out_bytes += std::min(frames[f].cap, y2j::stream_bound(frames[f].w, frames[f].h));
    }
    if (blocks >= ((size_t)1 << 31)) return fail(YOLO2_ERROR, "jpeg: %zu blocks in one chunk; use a smaller batch", blocks);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += padded(bytes); return o; };
    p.coef = take(blocks * 64 * sizeof(int16_t));
    p.blk_off = take(blocks * sizeof(uint32_t));
    p.wg_sum = take(groups * sizeof(uint32_t));
    p.wg_base = take(groups * sizeof(unsigned long long));
    p.us = take(us);
    p.seg_ff = take(segs * sizeof(uint32_t));
    p.seg_base = take(segs * sizeof(uint32_t));
    p.state = take((size_t)nf * sizeof(JpegState));
    p.sizes = take((size_t)nf * sizeof(unsigned long long));
    p.work_bytes = at;
    p.grid_blk = max_groups;
    p.grid_seg = std::min(max_segs, 64u);   // (segments beyond a workgroup's first are taken in a loop; real streams are far below the bound)
    *plan = p;
    return YOLO2_SUCCESS;
}

void y2_jpeg_write_table(const Y2JpegFrameIn *frames, int nf, int quality, uint8_t *table)
{
    memset(table, 0, y2_jpeg_table_bytes(nf));
    y2j::make_tables(quality, &reinterpret_cast<JpegHeader *>(table)->t);
    JpegFrame *jf = reinterpret_cast<JpegFrame *>(table + sizeof(JpegHeader));
    size_t blocks = 0, groups = 0, us = 0, segs = 0;
    for (int f = 0; f < nf; ++f) {
        const FrameShare s = frame_share(frames[f].w, frames[f].h);
        jf[f].src_off = frames[f].src_off;
        jf[f].us_off = us;
        jf[f].cap = frames[f].cap;
        jf[f].w = frames[f].w; jf[f].h = frames[f].h; jf[f].mcux = s.mcux; jf[f].n_blk = s.n_blk;
        jf[f].blk0 = (unsigned)blocks; jf[f].wg0 = (unsigned)groups; jf[f].n_wg = s.n_wg; jf[f].seg0 = (unsigned)segs;
        blocks += (size_t)s.n_blk;
        groups += s.n_wg;
        us += s.us_bytes;
        segs += s.n_seg;
    }
}

int y2_jpeg_enqueue(const Y2JpegPlan &p, const uint8_t *table_dev, const uint8_t *src_base, uint8_t *work, uint8_t *out_base, hipStream_t st)
{
    int16_t *coef = reinterpret_cast<int16_t *>(work + p.coef);
    uint32_t *blk_off = reinterpret_cast<uint32_t *>(work + p.blk_off), *wg_sum = reinterpret_cast<uint32_t *>(work + p.wg_sum);
    unsigned long long *wg_base = reinterpret_cast<unsigned long long *>(work + p.wg_base);
    uint8_t *us = work + p.us;
    uint32_t *seg_ff = reinterpret_cast<uint32_t *>(work + p.seg_ff), *seg_base = reinterpret_cast<uint32_t *>(work + p.seg_base);
    JpegState *state = reinterpret_cast<JpegState *>(work + p.state);
    unsigned long long *sizes = reinterpret_cast<unsigned long long *>(work + p.sizes);
    const dim3 per_blk(p.grid_blk, (unsigned)p.nf), per_seg(p.grid_seg, (unsigned)p.nf), per_frame((unsigned)p.nf);
    hipLaunchKernelGGL(k_jpeg_transform, per_blk, dim3(kJpegBlocks), 0, st, table_dev, src_base, coef);
    hipLaunchKernelGGL(k_jpeg_lengths, per_blk, dim3(kJpegBlocks), 0, st, table_dev, coef, blk_off, wg_sum);
    hipLaunchKernelGGL(k_jpeg_scan_groups, per_frame, dim3(kJpegScan), 0, st, table_dev, wg_sum, wg_base, us, state);
    hipLaunchKernelGGL(k_jpeg_pack, per_blk, dim3(kJpegBlocks), 0, st, table_dev, coef, blk_off, wg_sum, wg_base, us);
    hipLaunchKernelGGL(k_jpeg_count_ff, per_seg, dim3(kJpegSegThreads), 0, st, table_dev, us, state, seg_ff);
    hipLaunchKernelGGL(k_jpeg_scan_segs, per_frame, dim3(kJpegScan), 0, st, table_dev, seg_ff, seg_base, state, sizes);
    hipLaunchKernelGGL(k_jpeg_place, dim3(1), dim3(kJpegScan), 0, st, table_dev, state, p.nf);
    hipLaunchKernelGGL(k_jpeg_emit, per_seg, dim3(kJpegSegThreads), 0, st, table_dev, us, state, seg_base, out_base);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- one frame already on the device

extern "C" int yolo2_hip_jpeg_encode_rgb24(uint64_t rgb_dev, int w, int h, int quality, uint64_t jpeg_out_dev, size_t cap, size_t *size,
                                           void *stream)
{
    if (!rgb_dev || !size || (cap && !jpeg_out_dev)) return fail(YOLO2_ERROR, "jpeg: null argument");
    const Y2JpegFrameIn fr = {w, h, 0, cap};
    std::vector<uint8_t> tbl(y2_jpeg_table_bytes(1));
    Y2JpegPlan plan;
    int rc;
    if ((rc = y2_jpeg_plan(&fr, 1, &plan))) return rc;
    y2_jpeg_write_table(&fr, 1, quality, tbl.data());
    Y2DevBuf<uint8_t> dtbl, work;
    if ((rc = dtbl.alloc(tbl.size())) || (rc = work.alloc(plan.work_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(dtbl.get(), tbl.data(), tbl.size(), hipMemcpyHostToDevice, st), YOLO2_DMA_ERROR);
    if ((rc = y2_jpeg_enqueue(plan, dtbl.get(), (const uint8_t *)(uintptr_t)rgb_dev, work.get(), (uint8_t *)(uintptr_t)jpeg_out_dev, st))) return rc;
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, work.get() + plan.sizes, sizeof(n), hipMemcpyDeviceToHost, st), YOLO2_DMA_ERROR);
    HIP_TRY(hipStreamSynchronize(st), YOLO2_ERROR);
    *size = (size_t)n;
    if (n > cap) return fail(YOLO2_ERROR, "jpeg: output buffer too small (%zu < %llu bytes)", cap, n);
    return YOLO2_SUCCESS;
}
