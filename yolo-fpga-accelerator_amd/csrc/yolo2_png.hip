// yolo2_png.hip -- bytes in device memory -> zlib streams (include/yolo2_hip.h, "annotated frames as PNG"): the deflate stage of the
// library's own PNG definition (csrc/png_huff.hpp), made by the six launches of kernels_png.hpp.  The host side here lays the work
// area out and enqueues; nothing is read back between the stages.  host/y2_png.cpp writes the same bytes on the host.
#include "y2_internal.hpp"
#include "kernels_png.hpp"
#include "y2_png.hpp"

using namespace y2;

namespace {
size_t padded(size_t b, size_t to = 256) { return (b + to - 1) / to * to; }
}  // namespace

extern "C" size_t yolo2_hip_zlib_huff_bound(size_t n) { return y2p::zlib_bound(n); }

int y2_png_plan(const Y2PngIn *in, int nf, Y2PngPlan *plan)
{
    Y2PngPlan p;
    p.nf = nf;
    p.table.assign(padded((size_t)nf * sizeof(PngStream)), 0);
    PngStream *ps = reinterpret_cast<PngStream *>(p.table.data());
    size_t at = 0, blocks = 0;
    auto take = [&](size_t bytes, size_t to = 256) { const size_t o = at; at += padded(bytes, to); return o; };
    for (int f = 0; f < nf; ++f) {
        PngStream &s = ps[f];
        s.n = in[f].n;
        s.src_off = in[f].src_off; s.out_off = in[f].out_off;
        s.ds_off = take(y2p::zlib_bound(s.n) + 8, kPngTile);   // (k_png_emit reads whole tiles)
        s.blk0 = (uint32_t)blocks; s.n_blk = (uint32_t)y2p::n_blocks(s.n);
        blocks += s.n_blk;
        if (blocks >= ((size_t)1 << 31)) return fail(YOLO2_ERROR, "png: %zu deflate blocks in one chunk; use a smaller batch", blocks);
        p.grid_blk = std::max(p.grid_blk, s.n_blk);
        p.grid_tile = std::max(p.grid_tile, (unsigned)((y2p::zlib_bound(s.n) + kPngTile - 1) / kPngTile));
    }
    p.total_blocks = (unsigned)blocks;
    p.hist = take(blocks * y2p::kLitSyms * sizeof(uint32_t));
    p.codes = take(blocks * y2p::kLitSyms * sizeof(uint32_t));
    p.hdr = take(blocks * y2p::kHdrBytes);
    p.blocks = take(blocks * sizeof(PngBlock));
    p.state = take((size_t)nf * sizeof(PngState));
    p.sizes = take((size_t)nf * sizeof(unsigned long long));
    p.work_bytes = at;
    *plan = std::move(p);
    return YOLO2_SUCCESS;
}

int y2_png_enqueue(const Y2PngPlan &p, const uint8_t *table_dev, const uint8_t *src_base, uint8_t *work, uint8_t *out_base, hipStream_t st)
{
    const PngStream *streams = reinterpret_cast<const PngStream *>(table_dev);
    uint32_t *hist = reinterpret_cast<uint32_t *>(work + p.hist), *codes = reinterpret_cast<uint32_t *>(work + p.codes);
    uint8_t *hdr = work + p.hdr;
    PngBlock *blocks = reinterpret_cast<PngBlock *>(work + p.blocks);
    PngState *state = reinterpret_cast<PngState *>(work + p.state);
    unsigned long long *sizes = reinterpret_cast<unsigned long long *>(work + p.sizes);
    const dim3 per_blk(p.grid_blk, (unsigned)p.nf), per_stream((unsigned)(p.nf + 63) / 64);
    hipLaunchKernelGGL(k_png_hist, per_blk, dim3(kPngThreads), 0, st, streams, src_base, work, hist, blocks);
    hipLaunchKernelGGL(k_png_codes, dim3((p.total_blocks + kPngWaves - 1) / kPngWaves), dim3(kPngThreads), 0, st, hist, codes, hdr, blocks, p.total_blocks);
    hipLaunchKernelGGL(k_png_scan, per_stream, dim3(64), 0, st, streams, p.nf, blocks, work, state);
    hipLaunchKernelGGL(k_png_pack, per_blk, dim3(kPngThreads), 0, st, streams, src_base, work, codes, hdr, blocks);
    hipLaunchKernelGGL(k_png_emit, dim3(p.grid_tile, (unsigned)p.nf), dim3(kPngThreads), 0, st, streams, work, state, out_base);
    hipLaunchKernelGGL(k_png_finish, per_stream, dim3(64), 0, st, streams, p.nf, state, out_base, sizes);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- one stream already on the device

namespace {
int encode_one(const Y2PngIn &in, uint64_t src_dev, uint64_t out_dev, size_t *size, hipStream_t st)
{
    Y2PngPlan plan;
    int rc;
    if ((rc = y2_png_plan(&in, 1, &plan))) return rc;
    Y2DevBuf<uint8_t> dtbl, work;
    if ((rc = dtbl.alloc(plan.table.size())) || (rc = work.alloc(plan.work_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(dtbl.get(), plan.table.data(), plan.table.size(), hipMemcpyHostToDevice, st), YOLO2_DMA_ERROR);
    if ((rc = y2_png_enqueue(plan, dtbl.get(), (const uint8_t *)(uintptr_t)src_dev, work.get(), (uint8_t *)(uintptr_t)out_dev, st))) return rc;
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, work.get() + plan.sizes, sizeof(n), hipMemcpyDeviceToHost, st), YOLO2_DMA_ERROR);
    HIP_TRY(hipStreamSynchronize(st), YOLO2_ERROR);
    *size = (size_t)n;
    return YOLO2_SUCCESS;
}
}  // namespace

extern "C" int yolo2_hip_zlib_huff(uint64_t in_dev, size_t n, uint64_t out_dev, size_t cap, size_t *size)
{
    if ((n && !in_dev) || !size || !out_dev) return fail(YOLO2_ERROR, "zlib_huff: null argument");
    if (n >= ((size_t)1 << 31)) return fail(YOLO2_ERROR, "zlib_huff: %zu bytes; the entry takes less than 2 GiB", n);
    if (cap < y2p::zlib_bound(n))
        return fail(YOLO2_ERROR, "zlib_huff: output buffer too small (%zu < %zu bytes, yolo2_hip_zlib_huff_bound)", cap, y2p::zlib_bound(n));
    const Y2PngIn in = {n, 0, 0};
    return encode_one(in, in_dev, out_dev, size, nullptr);
}
