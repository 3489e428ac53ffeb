// yolo2_draw.hip -- annotated frames (include/yolo2_hip.h, "annotated frames"): detection records + the frames they came from ->
// RGB24 frames with the boxes and tags of the reference's yolo2_draw_detections_rgb24 painted in, bit-identical.
//
// The host turns records into draw items (draw_list.hpp: corner casts, "%s %.2f" through the host's snprintf, glyph indices), the
// items travel with the frame bytes, and k_annotate_batch (kernels_draw.hpp) converts and paints in one pass per pixel.  One entry
// serves the records of every precision: it needs the frames and the records, no weights.  For the loop entry (yolo2_loop.hip) the
// items are made on the device instead, from records that never left it (k_draw_items; the y2_loop_* functions below).
#include "y2_internal.hpp"
#include "kernels_draw.hpp"
#include "y2_draw.hpp"
#include "y2_jpeg.hpp"

#include <cmath>

using namespace y2;
using y2d::DrawDet;

static_assert(sizeof(DrawDet) == sizeof(yolo2_hip_det), "draw_list.hpp restates yolo2_hip_det");

namespace {

size_t padded(size_t b) { return (b + 255) & ~(size_t)255; }

int check_geometry(int w, int h, const Y2PixDesc &pd, int frame)
{
    if (w <= 0 || h <= 0) return fail(YOLO2_ERROR, "annotate: bad frame size %dx%d (frame %d)", w, h, frame);
    if ((long)w * h > (1L << 28)) return fail(YOLO2_ERROR, "annotate: frame %d too large (%dx%d)", frame, w, h);
    return y2_pix_check_parity(pd, w, h, "annotate", frame);
}

int check_records(const yolo2_hip_det *dets, int n, int frame)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(dets[i].prob)) return fail(YOLO2_ERROR, "annotate: record %d of frame %d has a non-finite prob", i, frame);
    return YOLO2_SUCCESS;
}

int check_common(float thresh, int n_labels)
{
    if (!(thresh >= 0.f)) return fail(YOLO2_ERROR, "annotate: thresh %g is negative or not a number", (double)thresh);
    if (n_labels < 0) return fail(YOLO2_ERROR, "annotate: negative label count %d", n_labels);
    return YOLO2_SUCCESS;
}

// the records of one frame that are drawn (draw_make_item's rule), without making the items
int count_drawn(const yolo2_hip_det *dets, int n, float thresh)
{
    int k = 0;
    for (int i = 0; i < n; ++i) k += dets[i].prob > thresh && dets[i].cls >= 0;
    return k;
}

// One chunk's table at `tbl` (table_bytes(nf, items) bytes): header, frames, items.  src_off / out_off / geometry of each frame
// come from the caller; this fills the items and their ranges.  drawn (optional) [nf].
struct FrameIn {
    int w, h, ch;
    size_t src_off, out_off;
    const yolo2_hip_det *dets;
    int n_dets;
};
size_t table_bytes(int nf, size_t items)
{
    return padded(sizeof(AnnoHeader) + (size_t)nf * sizeof(AnnoFrame)) + padded(items * sizeof(DrawItem));
}
int fill_table(uint8_t *tbl, const FrameIn *fr, int nf, float thresh, const char *const *labels, int n_labels, int *drawn)
{
    AnnoHeader *hd = reinterpret_cast<AnnoHeader *>(tbl);
    for (int i = 0; i < y2d::kDrawGlyphs; ++i) hd->font[i] = y2d::kDrawFont[i];
    hd->items_off = padded(sizeof(AnnoHeader) + (size_t)nf * sizeof(AnnoFrame));
    AnnoFrame *af = reinterpret_cast<AnnoFrame *>(tbl + sizeof(AnnoHeader));
    DrawItem *items = reinterpret_cast<DrawItem *>(tbl + hd->items_off);
    int at = 0, max_strips = 0;
    for (int f = 0; f < nf; ++f) {
        af[f].src_off = fr[f].src_off;
        af[f].out_off = fr[f].out_off;
        af[f].w = fr[f].w; af[f].h = fr[f].h; af[f].ch = fr[f].ch;
        af[f].item0 = at;
        for (int i = 0; i < fr[f].n_dets; ++i) {
            DrawDet d;
            memcpy(&d, &fr[f].dets[i], sizeof(d));
            if (y2d::draw_make_item(d, fr[f].w, fr[f].h, thresh, labels, n_labels, &items[at])) ++at;
        }
        af[f].n_items = at - af[f].item0;
        af[f].strips = (int)(((long)fr[f].w * fr[f].h + kAnnoStripPx - 1) / kAnnoStripPx);
        max_strips = std::max(max_strips, af[f].strips);
        if (drawn) drawn[f] = af[f].n_items;
    }
    return max_strips;
}

// out_format: YOLO2_LOOP_OUT_RGB24 (the annotate entries' only form), _BGR24, or _NV12 / _I420, whose max_strips is the most
// anno_yuv_groups of a frame (y2_loop_fill_geom)
void launch_annotate(const uint8_t *table_dev, const uint8_t *src_base, uint8_t *out_base, int max_strips, int nf, hipStream_t st,
                     int out_format = YOLO2_LOOP_OUT_RGB24)
{
    auto *kernel = out_format == YOLO2_LOOP_OUT_BGR24 ? k_annotate_batch_bgr : out_format == YOLO2_LOOP_OUT_NV12 ? k_annotate_batch_nv12
                   : out_format == YOLO2_LOOP_OUT_I420 ? k_annotate_batch_i420 : k_annotate_batch;
    hipLaunchKernelGGL(kernel, dim3((unsigned)max_strips, (unsigned)nf), dim3(kAnnoThreads), 0, st, table_dev, src_base, out_base);
}

}  // namespace

// ---------------------------------------------------------------------------- one image already on the device

extern "C" int yolo2_hip_annotate_pix(uint64_t image_dev, int w, int h, int pixfmt, const yolo2_hip_det *dets, int n_dets, float thresh,
                                      const char *const *labels, int n_labels, uint64_t rgb_out_dev, int *drawn, void *stream)
{
    if (!image_dev || !rgb_out_dev) return fail(YOLO2_ERROR, "annotate: null buffer address");
    if (n_dets < 0 || (n_dets > 0 && !dets)) return fail(YOLO2_ERROR, "annotate: null records (n_dets %d)", n_dets);
    const Y2PixDesc *pd = y2_pix_desc(pixfmt, "annotate");
    if (!pd) return YOLO2_ERROR;
    const int ch = pd->ch;
    int rc;
    if ((rc = check_geometry(w, h, *pd, 0)) || (rc = check_common(thresh, n_labels)) || (rc = check_records(dets, n_dets, 0))) return rc;
    if (image_dev & (pd->align - 1)) return fail(YOLO2_ERROR, "annotate: a %s frame starts on a %u-byte boundary", pd->name, pd->align);
    const FrameIn fr = {w, h, ch, 0, 0, dets, n_dets};
    const size_t bytes = table_bytes(1, (size_t)count_drawn(dets, n_dets, thresh));
    std::vector<uint8_t> tbl(bytes);
    int n_drawn = 0;
    const int max_strips = fill_table(tbl.data(), &fr, 1, thresh, labels, n_labels, &n_drawn);
    Y2DevBuf<uint8_t> dtbl;
    if ((rc = dtbl.alloc(bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(dtbl.get(), tbl.data(), bytes, hipMemcpyHostToDevice, st), YOLO2_DMA_ERROR);
    launch_annotate(dtbl.get(), (const uint8_t *)(uintptr_t)image_dev, (uint8_t *)(uintptr_t)rgb_out_dev, max_strips, 1, st);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipStreamSynchronize(st), YOLO2_ERROR);
    if (drawn) *drawn = n_drawn;
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- n host images, chunks of `batch`

void y2_anno_free(yolo2_hip_ctx *c)
{
    Y2AnnoBufs &a = c->anno;
    for (int k = 0; k < 2; ++k)
        for (hipEvent_t *e : {&a.e_in[k], &a.e_run[k], &a.e_out[k]})
            if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    for (hipStream_t *s : {&a.s_in, &a.s_run, &a.s_out})
        if (*s) { (void)hipStreamDestroy(*s); *s = nullptr; }
    for (int k = 0; k < 2; ++k) { a.hin[k].reset(); a.hout[k].reset(); a.din[k].reset(); a.dout[k].reset(); }
    a.cap_in = a.cap_out = 0;
}

// two buffer sets of at least cap_in staging bytes (table + items + frames) and cap_out output bytes; three streams.  Grown on demand
// and kept with the context, like PipeBufs.
int y2_anno_ensure(yolo2_hip_ctx *c, size_t cap_in, size_t cap_out)
{
    Y2AnnoBufs &a = c->anno;
    if (a.s_in && a.cap_in >= cap_in && a.cap_out >= cap_out) return YOLO2_SUCCESS;
    cap_in = std::max(cap_in, a.cap_in);
    cap_out = std::max(cap_out, a.cap_out);
    y2_anno_free(c);
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k)
        ok = a.hin[k].alloc(cap_in) == YOLO2_SUCCESS && a.din[k].alloc(cap_in) == YOLO2_SUCCESS && a.hout[k].alloc(cap_out) == YOLO2_SUCCESS &&
             a.dout[k].alloc(cap_out) == YOLO2_SUCCESS && hipEventCreateWithFlags(&a.e_in[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&a.e_run[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&a.e_out[k], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&a.s_in, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&a.s_run, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&a.s_out, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        y2_anno_free(c);
        return fail(YOLO2_MMAP_ERROR, "annotate: staging buffers (%zu + %zu bytes, twice) could not be allocated", cap_in, cap_out);
    }
    a.cap_in = cap_in;
    a.cap_out = cap_out;
    return YOLO2_SUCCESS;
}

// (y2_draw.hpp)
int y2_annotate_check(const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch, const yolo2_hip_det *dets,
                      int cap_per_frame, const int *counts, float thresh, int n_labels, uint8_t *const *annotated)
{
    if (!images || !widths || !heights || !dets || !counts || !annotated) return fail(YOLO2_ERROR, "annotate: null argument");
    const Y2PixDesc *pd = y2_pix_desc(pixfmt, "annotate");
    if (!pd) return YOLO2_ERROR;
    if (n <= 0 || batch <= 0 || batch > 1024 || cap_per_frame <= 0)
        return fail(YOLO2_ERROR, "annotate: bad image count %d / batch %d (1..1024) / capacity %d", n, batch, cap_per_frame);
    int rc;
    if ((rc = check_common(thresh, n_labels))) return rc;
    for (int f = 0; f < n; ++f) {
        if (!images[f] || !annotated[f]) return fail(YOLO2_ERROR, "annotate: null image or output %d", f);
        if (counts[f] < 0) return fail(YOLO2_ERROR, "annotate: negative record count %d of frame %d", counts[f], f);
        if ((rc = check_geometry(widths[f], heights[f], *pd, f)) ||
            (rc = check_records(dets + (size_t)f * cap_per_frame, std::min(counts[f], cap_per_frame), f)))
            return rc;
    }
    return YOLO2_SUCCESS;
}

// Upload of chunk k + 1 (host staging copy, item making, DMA) overlaps the kernel of chunk k and the download of chunk k - 1: the
// three-stream pipeline of the images entries (yolo2_hip.hip), with the RGB24 frames as the product that comes back.
extern "C" int yolo2_hip_annotate_images_pix_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                                  int pixfmt, int n, int batch, const yolo2_hip_det *dets, int cap_per_frame,
                                                  const int *counts, float thresh, const char *const *labels, int n_labels,
                                                  uint8_t *const *annotated, int *drawn)
{
    if (!c) return fail(YOLO2_ERROR, "annotate: null argument");
    int rc;
    if ((rc = y2_annotate_check(images, widths, heights, pixfmt, n, batch, dets, cap_per_frame, counts, thresh, n_labels, annotated))) return rc;
    const int ch = y2_pix_desc(pixfmt, "annotate")->ch;
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    auto used = [&](int f) { return std::min(counts[f], cap_per_frame); };
    size_t cap_in = 0, cap_out = 0;
    for (int k = 0; k < chunks; ++k) {
        size_t items = 0, in = 0, out = 0;
        for (int f = k * batch; f < k * batch + in_chunk(k); ++f) {
            items += (size_t)count_drawn(dets + (size_t)f * cap_per_frame, used(f), thresh);
            in += padded(y2_frame_bytes(widths[f], heights[f], ch));
            out += padded((size_t)widths[f] * heights[f] * 3);
        }
        cap_in = std::max(cap_in, table_bytes(in_chunk(k), items) + in);
        cap_out = std::max(cap_out, out);
    }
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if ((rc = y2_anno_ensure(c, cap_in, cap_out))) return rc;
    Y2AnnoBufs &A = c->anno;
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)

    std::vector<FrameIn> fr((size_t)batch);
    auto drain = [&](int k) {
        const int b = k & 1;
        (void)hipEventSynchronize(A.e_out[b]);
        size_t off = 0;
        for (int f = k * batch; f < k * batch + in_chunk(k); ++f) {
            const size_t bytes = (size_t)widths[f] * heights[f] * 3;
            memcpy(annotated[f], A.hout[b].get() + off, bytes);
            off += padded(bytes);
        }
    };
    for (int k = 0; k < chunks; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        if (k >= 2) drain(k - 2);   // buffer set b is free again once chunk k-2 has left it
        size_t items = 0;
        for (int i = 0; i < nf; ++i) items += (size_t)count_drawn(dets + (size_t)(first + i) * cap_per_frame, used(first + i), thresh);
        uint8_t *hin = A.hin[b].get();
        size_t off = table_bytes(nf, items), out_off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i;
            const size_t bytes = y2_frame_bytes(widths[f], heights[f], ch);
            memcpy(hin + off, images[f], bytes);
            fr[(size_t)i] = {widths[f], heights[f], ch, off, out_off, dets + (size_t)f * cap_per_frame, used(f)};
            off += padded(bytes);
            out_off += padded((size_t)widths[f] * heights[f] * 3);
        }
        const int max_strips = fill_table(hin, fr.data(), nf, thresh, labels, n_labels, drawn ? drawn + first : nullptr);
        Y2_TRY(hipMemcpyAsync(A.din[b].get(), hin, off, hipMemcpyHostToDevice, A.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(A.e_in[b], A.s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(A.s_run, A.e_in[b], 0), YOLO2_ERROR);
        launch_annotate(A.din[b].get(), A.din[b].get(), A.dout[b].get(), max_strips, nf, A.s_run);
        Y2_TRY(hipGetLastError(), YOLO2_ERROR);
        Y2_TRY(hipEventRecord(A.e_run[b], A.s_run), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(A.s_out, A.e_run[b], 0), YOLO2_ERROR);
        Y2_TRY(hipMemcpyAsync(A.hout[b].get(), A.dout[b].get(), out_off, hipMemcpyDeviceToHost, A.s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(A.e_out[b], A.s_out), YOLO2_ERROR);
    }
    for (int k = std::max(0, chunks - 2); k < chunks; ++k) drain(k);
#undef Y2_TRY
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- the draw list on the device (the loop entry, yolo2_loop.hip)

void y2_loop_free(yolo2_hip_ctx *c)
{
    Y2LoopBufs &l = c->loop;
    l.table.reset(); l.labels.reset(); l.info.reset();
    for (int k = 0; k < 2; ++k) l.hinfo[k].reset();
    l.cap_table = l.cap_labels = l.cap_frames = 0;
}

size_t y2_loop_geom_bytes(int nf) { return padded(sizeof(AnnoHeader) + (size_t)nf * sizeof(AnnoFrame)); }

int y2_loop_fill_geom(uint8_t *geom, int nf, const int *widths, const int *heights, int ch, const size_t *src_off, const size_t *out_off, int out_format)
{
    const bool yuv = out_format == YOLO2_LOOP_OUT_NV12 || out_format == YOLO2_LOOP_OUT_I420;
    AnnoHeader *hd = reinterpret_cast<AnnoHeader *>(geom);
    for (int i = 0; i < y2d::kDrawGlyphs; ++i) hd->font[i] = y2d::kDrawFont[i];
    hd->items_off = y2_loop_geom_bytes(nf);
    AnnoFrame *af = reinterpret_cast<AnnoFrame *>(geom + sizeof(AnnoHeader));
    int max_strips = 0;
    for (int f = 0; f < nf; ++f) {
        af[f].src_off = src_off[f];
        af[f].out_off = out_off[f];
        af[f].w = widths[f]; af[f].h = heights[f]; af[f].ch = ch;
        af[f].item0 = af[f].n_items = 0;   // (k_draw_items fills them in the device's copy)
        af[f].strips = (int)(((long)widths[f] * heights[f] + kAnnoStripPx - 1) / kAnnoStripPx);
        max_strips = std::max(max_strips, yuv ? anno_yuv_groups(widths[f], heights[f]) : af[f].strips);   // (strips stays the flat count)
    }
    return max_strips;
}

// The context's scratch for chunks of up to `frames` frames with `cap` records each - the complete table (header, frames, cap items per
// frame; written and read by kernels of ONE stream, so one of it), the per-frame info and its two pinned mirrors - and the call's
// label table, uploaded here (synchronous: `labels` is the caller's).
int y2_loop_ensure(yolo2_hip_ctx *c, int frames, int cap, const char *const *labels, int n_labels)
{
    Y2LoopBufs &l = c->loop;
    int rc;
    const size_t need = y2_loop_geom_bytes(frames) + padded((size_t)frames * cap * sizeof(DrawItem));
    if (l.cap_table < need) {
        l.cap_table = 0;
        if ((rc = l.table.alloc(need))) return rc;
        l.cap_table = need;
    }
    if (l.cap_frames < frames) {
        l.cap_frames = 0;
        if ((rc = l.info.alloc((size_t)frames * 2))) return rc;
        for (int k = 0; k < 2; ++k)
            if ((rc = l.hinfo[k].alloc((size_t)frames * 2))) return rc;
        l.cap_frames = frames;
    }
    if (!labels) n_labels = 0;
    const size_t lbytes = (size_t)n_labels * y2d::kDrawLabelStride;
    if (lbytes) {
        if (l.cap_labels < lbytes) {
            l.cap_labels = 0;
            if ((rc = l.labels.alloc(lbytes))) return rc;
            l.cap_labels = lbytes;
        }
        std::vector<uint8_t> tbl(lbytes);
        for (int i = 0; i < n_labels; ++i) y2d::draw_label_entry(labels[i], tbl.data() + (size_t)i * y2d::kDrawLabelStride);
        HIP_TRY(hipMemcpy(l.labels.get(), tbl.data(), lbytes, hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    }
    return YOLO2_SUCCESS;
}

int y2_loop_enqueue_items(yolo2_hip_ctx *c, int b, int nf, int cap, float thresh, const char *const *labels, int n_labels, const uint8_t *geom_dev,
                          const yolo2_hip_det *dets_dev, const int *counts_dev, hipStream_t st)
{
    Y2LoopBufs &l = c->loop;
    if (nf > l.cap_frames || y2_loop_geom_bytes(nf) + (size_t)nf * cap * sizeof(DrawItem) > l.cap_table)
        return fail(YOLO2_ERROR, "loop: item scratch too small for %d frames x %d records", nf, cap);
    const bool with_labels = labels && n_labels > 0;
    hipLaunchKernelGGL(k_draw_items, dim3((unsigned)nf), dim3(kItemsThreads), 0, st, reinterpret_cast<const DrawDet *>(dets_dev), counts_dev, cap,
                       thresh, with_labels ? l.labels.get() : (const uint8_t *)nullptr, with_labels ? n_labels : 0, geom_dev, l.table.get(), l.info.get());
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpyAsync(l.hinfo[b].get(), l.info.get(), (size_t)nf * 2 * sizeof(int), hipMemcpyDeviceToHost, st), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

int y2_loop_enqueue_paint(yolo2_hip_ctx *c, int nf, int max_strips, const uint8_t *src_base, uint8_t *out_base, int out_format, hipStream_t st)
{
    launch_annotate(c->loop.table.get(), src_base, out_base, max_strips, nf, st, out_format);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// The test doorway: records and counts on the device -> the items k_draw_items makes of them, on the host.
extern "C" size_t yolo2_hip_draw_item_size(void) { return sizeof(DrawItem); }
extern "C" int yolo2_hip_draw_items_dev(yolo2_hip_ctx *c, uint64_t dets_dev, uint64_t counts_dev, int n_frames, int cap_per_frame,
                                        const int *widths, const int *heights, float thresh, const char *const *labels, int n_labels,
                                        void *items, int *n_items, int *unprintable)
{
    if (!c || !dets_dev || !counts_dev || !widths || !heights || !items || !n_items) return fail(YOLO2_ERROR, "draw items: null argument");
    if (n_frames <= 0 || n_frames > 1024 || cap_per_frame <= 0 || cap_per_frame > 65536)
        return fail(YOLO2_ERROR, "draw items: bad frame count %d (1..1024) / capacity %d (1..65536)", n_frames, cap_per_frame);
    int rc;
    if ((rc = check_common(thresh, n_labels))) return rc;
    for (int f = 0; f < n_frames; ++f)
        if ((rc = check_geometry(widths[f], heights[f], *y2_pix_desc_ch(3), f))) return rc;
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if ((rc = y2_loop_ensure(c, n_frames, cap_per_frame, labels, n_labels))) return rc;
    const size_t gbytes = y2_loop_geom_bytes(n_frames);
    std::vector<uint8_t> geom(gbytes);
    std::vector<size_t> zero((size_t)n_frames, 0);
    (void)y2_loop_fill_geom(geom.data(), n_frames, widths, heights, 3, zero.data(), zero.data(), YOLO2_LOOP_OUT_RGB24);
    Y2DevBuf<uint8_t> dgeom;
    if ((rc = dgeom.alloc(gbytes))) return rc;
    HIP_TRY(hipMemcpy(dgeom.get(), geom.data(), gbytes, hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    if ((rc = y2_loop_enqueue_items(c, 0, n_frames, cap_per_frame, thresh, labels, n_labels, dgeom.get(), (const yolo2_hip_det *)(uintptr_t)dets_dev,
                                    (const int *)(uintptr_t)counts_dev, nullptr)))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr), YOLO2_ERROR);
    const int *info = c->loop.hinfo[0].get();
    int bad_frame = -1;
    for (int f = 0; f < n_frames; ++f) {
        n_items[f] = info[2 * f];
        if (unprintable) unprintable[f] = info[2 * f + 1];
        if (info[2 * f + 1] && bad_frame < 0) bad_frame = f;
        if (n_items[f] < 0 || n_items[f] > cap_per_frame) return fail(YOLO2_ERROR, "draw items: frame %d reports %d items", f, n_items[f]);
        if (n_items[f])
            HIP_TRY(hipMemcpy(static_cast<uint8_t *>(items) + (size_t)f * cap_per_frame * sizeof(DrawItem),
                              c->loop.table.get() + gbytes + (size_t)f * cap_per_frame * sizeof(DrawItem), (size_t)n_items[f] * sizeof(DrawItem),
                              hipMemcpyDeviceToHost),
                    YOLO2_DMA_ERROR);
    }
    if (bad_frame >= 0) return fail(YOLO2_ERROR, "draw items: frame %d has a record with a non-finite (or 2^23 and larger) prob among those to be drawn", bad_frame);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- n host images -> annotated frames as JPEG streams

void y2_anno_jpeg_free(yolo2_hip_ctx *c)
{
    Y2JpegBufs &j = c->jpeg;
    for (int k = 0; k < 2; ++k) {
        if (j.e_sizes[k]) { (void)hipEventDestroy(j.e_sizes[k]); j.e_sizes[k] = nullptr; }
        j.dout[k].reset(); j.hout[k].reset(); j.hsizes[k].reset();
    }
    j.rgb.reset();
    j.work.reset();
    j.cap_rgb = j.cap_work = j.cap_out = j.cap_frames = 0;
}

int y2_anno_jpeg_ensure(yolo2_hip_ctx *c, size_t cap_rgb, size_t cap_work, size_t cap_out, size_t frames)
{
    Y2JpegBufs &j = c->jpeg;
    if (j.e_sizes[0] && j.cap_rgb >= cap_rgb && j.cap_work >= cap_work && j.cap_out >= cap_out && j.cap_frames >= frames) return YOLO2_SUCCESS;
    cap_rgb = std::max(cap_rgb, j.cap_rgb);
    cap_work = std::max(cap_work, j.cap_work);
    cap_out = std::max(cap_out, j.cap_out);
    frames = std::max(frames, j.cap_frames);
    y2_anno_jpeg_free(c);
    bool ok = j.rgb.alloc(cap_rgb) == YOLO2_SUCCESS && j.work.alloc(cap_work) == YOLO2_SUCCESS;
    for (int k = 0; k < 2 && ok; ++k)
        ok = j.dout[k].alloc(cap_out) == YOLO2_SUCCESS && j.hout[k].alloc(cap_out) == YOLO2_SUCCESS && j.hsizes[k].alloc(frames) == YOLO2_SUCCESS &&
             hipEventCreateWithFlags(&j.e_sizes[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        y2_anno_jpeg_free(c);
        return fail(YOLO2_MMAP_ERROR, "annotate: JPEG buffers (%zu + %zu bytes, and %zu twice) could not be allocated", cap_rgb, cap_work, cap_out);
    }
    j.cap_rgb = cap_rgb; j.cap_work = cap_work; j.cap_out = cap_out; j.cap_frames = frames;
    return YOLO2_SUCCESS;
}

// (y2_draw.hpp)
int y2_annotate_jpeg_check(const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch,
                           const yolo2_hip_det *dets, int cap_per_frame, const int *counts, float thresh, int n_labels, uint8_t *const *jpeg,
                           const size_t *caps, size_t *sizes)
{
    if (!caps || !sizes) return fail(YOLO2_ERROR, "annotate: null argument");
    int rc;
    if ((rc = y2_annotate_check(images, widths, heights, pixfmt, n, batch, dets, cap_per_frame, counts, thresh, n_labels, jpeg))) return rc;
    for (int f = 0; f < n; ++f)
        if ((rc = y2_jpeg_check_frame(widths[f], heights[f], f))) return rc;
    return YOLO2_SUCCESS;
}

// The painter's pipeline with the encoder behind it on the run stream: chunk k's frames are painted into device memory
// (k_annotate_batch), encoded there (stages A - D of kernels_jpeg.hpp) and only the streams come back - first the sizes, then one copy
// of the bytes in use.  While the GPU paints and encodes chunk k, the output stream downloads chunk k - 1's bytes and the host copies
// them out of pinned memory: the byte copy of chunk k - 1 is queued on the output stream BEFORE that stream is made to wait for chunk
// k's kernels (for chunk k's sizes copy).
extern "C" int yolo2_hip_annotate_images_pix_jpeg_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                                       int pixfmt, int n, int batch, const yolo2_hip_det *dets, int cap_per_frame,
                                                       const int *counts, float thresh, const char *const *labels, int n_labels, int quality,
                                                       uint8_t *const *jpeg, const size_t *caps, size_t *sizes, int *drawn)
{
    if (!c) return fail(YOLO2_ERROR, "annotate: null argument");
    int rc;
    if ((rc = y2_annotate_jpeg_check(images, widths, heights, pixfmt, n, batch, dets, cap_per_frame, counts, thresh, n_labels, jpeg, caps, sizes)))
        return rc;
    const int ch = y2_pix_desc(pixfmt, "annotate")->ch;
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    auto used = [&](int f) { return std::min(counts[f], cap_per_frame); };
    // per chunk: the painter's item count and the encoder's plan, made once; an upload holds the painter's table, the frames, then
    // the encoder's table
    std::vector<Y2JpegFrameIn> jf((size_t)batch);
    std::vector<Y2JpegPlan> plans((size_t)chunks);
    std::vector<size_t> items((size_t)chunks, 0);
    size_t cap_in = 0, cap_rgb = 0, cap_work = 0, cap_out = 0;
    for (int k = 0; k < chunks; ++k) {
        size_t in = 0, out = 0;
        for (int i = 0; i < in_chunk(k); ++i) {
            const int f = k * batch + i;
            items[(size_t)k] += (size_t)count_drawn(dets + (size_t)f * cap_per_frame, used(f), thresh);
            in += padded(y2_frame_bytes(widths[f], heights[f], ch));
            jf[(size_t)i] = {widths[f], heights[f], out, caps[f]};
            out += padded((size_t)widths[f] * heights[f] * 3);
        }
        if ((rc = y2_jpeg_plan(jf.data(), in_chunk(k), &plans[(size_t)k]))) return rc;
        cap_in = std::max(cap_in, table_bytes(in_chunk(k), items[(size_t)k]) + in + plans[(size_t)k].table_bytes);
        cap_rgb = std::max(cap_rgb, out);
        cap_work = std::max(cap_work, plans[(size_t)k].work_bytes);
        cap_out = std::max(cap_out, plans[(size_t)k].out_bytes);
    }
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if ((rc = y2_anno_ensure(c, cap_in, 0)) || (rc = y2_anno_jpeg_ensure(c, cap_rgb, cap_work, std::max(cap_out, (size_t)1), (size_t)batch))) return rc;
    Y2AnnoBufs &A = c->anno;
    Y2JpegBufs &J = c->jpeg;
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)

    std::vector<FrameIn> fr((size_t)batch);
    int short_frame = -1;
    // The sizes first, then only the bytes in use: frame f's stream starts where the frames before it end, each cut at its capacity.
    // fetch(k): wait for chunk k's sizes, queue one D2H of the bytes in use.  deliver(k): wait for it, hand the streams out.
    auto fetch = [&](int k) -> int {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        Y2_TRY(hipEventSynchronize(J.e_sizes[b]), YOLO2_ERROR);
        const unsigned long long *hs = J.hsizes[b].get();
        size_t total = 0;
        for (int i = 0; i < nf; ++i) total += std::min((size_t)hs[i], caps[first + i]);
        if (total) Y2_TRY(hipMemcpyAsync(J.hout[b].get(), J.dout[b].get(), total, hipMemcpyDeviceToHost, A.s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(A.e_out[b], A.s_out), YOLO2_ERROR);
        return YOLO2_SUCCESS;
    };
    auto deliver = [&](int k) -> int {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        Y2_TRY(hipEventSynchronize(A.e_out[b]), YOLO2_ERROR);
        const unsigned long long *hs = J.hsizes[b].get();
        size_t off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i;
            const size_t bytes = std::min((size_t)hs[i], caps[f]);
            if (bytes) memcpy(jpeg[f], J.hout[b].get() + off, bytes);
            off += bytes;
            sizes[f] = (size_t)hs[i];
            if (sizes[f] > caps[f] && short_frame < 0) short_frame = f;
        }
        return YOLO2_SUCCESS;
    };
    for (int k = 0; k < chunks; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        const Y2JpegPlan &plan = plans[(size_t)k];
        // (buffer set b is free: chunk k - 2 was delivered in the round before)
        uint8_t *hin = A.hin[b].get();
        size_t off = table_bytes(nf, items[(size_t)k]), out_off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i;
            const size_t bytes = y2_frame_bytes(widths[f], heights[f], ch);
            memcpy(hin + off, images[f], bytes);
            fr[(size_t)i] = {widths[f], heights[f], ch, off, out_off, dets + (size_t)f * cap_per_frame, used(f)};
            jf[(size_t)i] = {widths[f], heights[f], out_off, caps[f]};
            off += padded(bytes);
            out_off += padded((size_t)widths[f] * heights[f] * 3);
        }
        const int max_strips = fill_table(hin, fr.data(), nf, thresh, labels, n_labels, drawn ? drawn + first : nullptr);
        const size_t jtab = off;
        y2_jpeg_write_table(jf.data(), nf, quality, hin + jtab);
        off += plan.table_bytes;
        Y2_TRY(hipMemcpyAsync(A.din[b].get(), hin, off, hipMemcpyHostToDevice, A.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(A.e_in[b], A.s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(A.s_run, A.e_in[b], 0), YOLO2_ERROR);
        // (the work area holds the sizes of the chunk before until they have been copied out)
        if (k >= 1) Y2_TRY(hipStreamWaitEvent(A.s_run, J.e_sizes[b ^ 1], 0), YOLO2_ERROR);
        launch_annotate(A.din[b].get(), A.din[b].get(), J.rgb.get(), max_strips, nf, A.s_run);
        Y2_TRY(hipGetLastError(), YOLO2_ERROR);
        if ((rc = y2_jpeg_enqueue(plan, A.din[b].get() + jtab, J.rgb.get(), J.work.get(), J.dout[b].get(), A.s_run))) { cleanup(); return rc; }
        Y2_TRY(hipEventRecord(A.e_run[b], A.s_run), YOLO2_ERROR);
        // chunk k - 1's bytes go onto the output stream ahead of the wait for chunk k's kernels, so they come down while those run
        if (k >= 1 && (rc = fetch(k - 1))) return rc;
        Y2_TRY(hipStreamWaitEvent(A.s_out, A.e_run[b], 0), YOLO2_ERROR);
        Y2_TRY(hipMemcpyAsync(J.hsizes[b].get(), J.work.get() + plan.sizes, (size_t)nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, A.s_out),
               YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(J.e_sizes[b], A.s_out), YOLO2_ERROR);
        if (k >= 1 && (rc = deliver(k - 1))) return rc;
    }
    if ((rc = fetch(chunks - 1)) || (rc = deliver(chunks - 1))) return rc;
#undef Y2_TRY
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    if (short_frame >= 0)
        return fail(YOLO2_ERROR, "annotate: output buffer too small for frame %d (%zu < %zu bytes)", short_frame, caps[short_frame], sizes[short_frame]);
    return YOLO2_SUCCESS;
}
