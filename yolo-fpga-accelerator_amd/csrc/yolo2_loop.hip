// yolo2_loop.hip -- the camera loop as one call (include/yolo2_hip.h, "the camera loop as one call"): frames -> detection records AND
// the annotated frames (RGB24 or JPEG) from ONE upload per chunk.
//
// It joins what the images -> detections entries (yolo2_hip.hip) and the annotate entries (yolo2_draw.hip) do in two calls, on the
// device: the chunk's frames stay in PipeBufs' device staging buffer from the letterbox to the painter, the records stay in HBM from
// k_compact_dets to the painter, and the draw items - the one thing the two-call route makes on the host - come from k_draw_items.
//
// A chunk's staging buffer:  LetterboxItem[batch] | the painter's table as the host knows it (AnnoHeader, AnnoFrame[batch]) | the
// frames, each padded to 256 bytes | with JPEG out, the encoder's table.  One H2D.
//
// Streams (PipeBufs', double-buffered as run_images_i16_dets / run_images_f16):
//   s_in    the H2D of chunk k (staging + the tail's geometry records)
//   s_run   (or the int16 lanes' streams) letterbox + network of chunk k
//   s_out   tail -> k_draw_items -> k_annotate_batch -> [encoder] -> D2H of counts, records, item counts and the frames (or sizes)
//
// Ordering.  (1) Buffer set b (pinned staging hin[b], device staging dbytes[b], the tail's buffers, the pinned mirrors) is refilled
// for chunk k + 2 only after deliver(k) has waited for e_out[b], which is recorded on s_out behind chunk k's painter (and encoder, and
// copies): the painter runs on s_out, so the frames it reads from dbytes[b] cannot be overwritten under it.  (2) The painter table,
// the item counts, the painted frames of the JPEG route and the encoder's work area exist once: every kernel that touches them runs on
// s_out, which keeps chunks in order.  (3) With JPEG out the sizes come back first; the host reads them and queues ONE copy of the
// bytes in use.  That copy for chunk k - 1 is queued on s_out BEFORE s_out is made to wait for chunk k's network, so it runs while the
// network does, and the work area's sizes are copied out before chunk k's encoder (same stream) overwrites them.
#include "y2_internal.hpp"
#include "letterbox.hpp"
#include "y2_draw.hpp"
#include "y2_jpeg.hpp"

using namespace y2;

namespace {
size_t padded(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

// (y2_draw.hpp) everything the loop entries refuse that can be seen without a context
int y2_loop_check(int precision, const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch, float thresh,
                  int flags, const yolo2_hip_det *dets, int cap_per_frame, const int *counts, int n_labels, int out_format, int quality,
                  uint8_t *const *out, const size_t *caps, const size_t *sizes)
{
    if (!images || !widths || !heights || !dets || !counts || !out || !caps || !sizes) return fail(YOLO2_ERROR, "loop: null argument");
    if (precision != YOLO2_LOOP_INT16 && precision != YOLO2_LOOP_FP16 && precision != YOLO2_LOOP_F32TOL)
        return fail(YOLO2_ERROR, "loop: unknown precision %d (YOLO2_LOOP_INT16, _FP16 or _F32TOL)", precision);
    if (out_format != YOLO2_LOOP_OUT_RGB24 && out_format != YOLO2_LOOP_OUT_JPEG)
        return fail(YOLO2_ERROR, "loop: unknown output format %d (YOLO2_LOOP_OUT_RGB24 or _JPEG)", out_format);
    if (!(flags & YOLO2_DETS_BEST_CLASS)) return fail(YOLO2_ERROR, "loop: flags must contain YOLO2_DETS_BEST_CLASS, the form the painter draws");
    const int ch = y2_pix_channels(pixfmt);
    if (!ch) return YOLO2_ERROR;
    if (n <= 0 || batch <= 0 || batch > 1024 || cap_per_frame <= 0 || cap_per_frame > 65536)
        return fail(YOLO2_ERROR, "loop: bad image count %d / batch %d (1..1024) / capacity %d (1..65536)", n, batch, cap_per_frame);
    if (!(thresh >= 0.f)) return fail(YOLO2_ERROR, "loop: thresh %g is negative or not a number", (double)thresh);
    if (n_labels < 0) return fail(YOLO2_ERROR, "loop: negative label count %d", n_labels);
    if (out_format == YOLO2_LOOP_OUT_JPEG && (quality < 1 || quality > 100)) return fail(YOLO2_ERROR, "loop: JPEG quality %d outside 1..100", quality);
    for (int f = 0; f < n; ++f) {
        if (!images[f] || (!out[f] && caps[f])) return fail(YOLO2_ERROR, "loop: null image or output %d", f);
        LetterboxArgs a;
        int rc;
        if ((rc = y2_letterbox_args(widths[f], heights[f], ch, 416, 416, a, true))) return rc;
        if (out_format == YOLO2_LOOP_OUT_JPEG) {
            if ((rc = y2_jpeg_check_frame(widths[f], heights[f], f))) return rc;
        } else if (caps[f] < (size_t)widths[f] * heights[f] * 3) {
            return fail(YOLO2_ERROR, "loop: output buffer too small for frame %d (%zu < %zu bytes)", f, caps[f], (size_t)widths[f] * heights[f] * 3);
        }
    }
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_loop_last_info(yolo2_hip_ctx *c, yolo2_hip_loop_info_t *info)
{
    if (!c || !info) return fail(YOLO2_ERROR, "loop: null argument");
    *info = c->loop_info;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_loop_images_pix(yolo2_hip_ctx *c, int precision, const uint8_t *const *images, const int *widths, const int *heights,
                                         int pixfmt, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap,
                                         int *counts, int *final_q, const char *const *labels, int n_labels, int out_format, int quality,
                                         uint8_t *const *out, const size_t *caps, size_t *sizes, int *drawn)
{
    if (!c) return fail(YOLO2_ERROR, "loop: null argument");
    int rc;
    if ((rc = y2_loop_check(precision, images, widths, heights, pixfmt, n, batch, thresh, flags, dets, cap, counts, n_labels, out_format, quality, out,
                            caps, sizes)))
        return rc;
    const bool i16 = precision == YOLO2_LOOP_INT16, jpeg = out_format == YOLO2_LOOP_OUT_JPEG;
    const int split = precision == YOLO2_LOOP_F32TOL ? 1 : 0, ch = y2_pix_channels(pixfmt), app_tail = (flags & YOLO2_DETS_APP_TAIL) ? 1 : 0;
    const bool yuyv = ch == 2;
    if (i16 && !c->weights_loaded) return fail(YOLO2_ERROR, "loop: int16 weights not loaded");
    if (!i16 && (!c->f16_loaded || !c->f16_plan || !c->wf32)) return fail(YOLO2_ERROR, "loop: fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    yolo2_hip_ctx *run = nullptr;
    if (!i16 && (rc = y2_f16_images_ctx(c, split, &run))) return rc;
    const bool fused = !i16 && y2_f16_images_fused(run);

    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    const size_t lb_bytes = padded((size_t)batch * sizeof(LetterboxItem)), geom_bytes = y2_loop_geom_bytes(batch), lead = lb_bytes + geom_bytes;
    // per chunk: the staging bytes, the painted frames' bytes and (JPEG) the encoder's plan
    std::vector<Y2JpegFrameIn> jf((size_t)batch);
    std::vector<Y2JpegPlan> plans(jpeg ? (size_t)chunks : 0);
    size_t cap_in = 0, cap_rgb = 0, cap_work = 0, cap_out = 0;
    for (int k = 0; k < chunks; ++k) {
        size_t in = lead, rgb = 0;
        for (int i = 0; i < in_chunk(k); ++i) {
            const int f = k * batch + i;
            in += padded((size_t)widths[f] * heights[f] * ch);
            jf[(size_t)i] = {widths[f], heights[f], rgb, caps[f]};
            rgb += padded((size_t)widths[f] * heights[f] * 3);
        }
        if (jpeg) {
            if ((rc = y2_jpeg_plan(jf.data(), in_chunk(k), &plans[(size_t)k]))) return rc;
            in += plans[(size_t)k].table_bytes;
            cap_work = std::max(cap_work, plans[(size_t)k].work_bytes);
            cap_out = std::max(cap_out, plans[(size_t)k].out_bytes);
        }
        cap_in = std::max(cap_in, in);
        cap_rgb = std::max(cap_rgb, rgb);
    }
    if (i16 && batch != c->batch && (rc = yolo2_hip_set_batch(c, batch))) return rc;
    if ((rc = y2_pipe_ensure(c->pipe, cap_in, cap_in, batch, false)) || (rc = y2_pipe_ensure_post(c, batch, cap))) return rc;
    if (!i16 && (rc = y2_pipe_ensure_regf(c->pipe, batch, false))) return rc;
    if ((rc = y2_loop_ensure(c, batch, cap, labels, n_labels))) return rc;
    // the product's buffers are the annotate entries': two sets of device + pinned RGB24 frames, or the painted frames and the
    // encoder's work area once with two sets of packed streams and pinned sizes
    if (jpeg) rc = y2_anno_jpeg_ensure(c, cap_rgb, cap_work, std::max(cap_out, (size_t)1), (size_t)batch);
    else rc = y2_anno_ensure(c, 0, cap_rgb);
    if (rc) return rc;
    PipeBufs &P = c->pipe;
    Y2AnnoBufs &A = c->anno;
    Y2JpegBufs &J = c->jpeg;
    Y2LoopBufs &L = c->loop;
    yolo2_hip_loop_info_t info = {};
    snprintf(info.items_kernel, sizeof(info.items_kernel), "k_draw_items");
    const size_t gbytes = y2_post_geom_bytes();
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)

    int short_frame = -1, bad_frame = -1, q = 0;
    // fetch(k) (JPEG): wait for chunk k's sizes, queue one D2H of the stream bytes in use.  deliver(k): wait for chunk k's last copy and
    // hand everything out.
    auto fetch = [&](int k) -> int {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        Y2_TRY(hipEventSynchronize(J.e_sizes[b]), YOLO2_ERROR);
        const unsigned long long *hs = J.hsizes[b].get();
        size_t total = 0;
        for (int i = 0; i < nf; ++i) total += std::min((size_t)hs[i], caps[first + i]);
        if (total) Y2_TRY(hipMemcpyAsync(J.hout[b].get(), J.dout[b].get(), total, hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_out[b], P.s_out), YOLO2_ERROR);
        info.out_bytes_d2h += total + (size_t)nf * sizeof(unsigned long long);
        return YOLO2_SUCCESS;
    };
    auto deliver = [&](int k) -> int {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        Y2_TRY(hipEventSynchronize(P.e_out[b]), YOLO2_ERROR);
        memcpy(counts + first, P.hcounts[b].get(), (size_t)nf * sizeof(int));
        size_t off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i, cnt = std::min(std::max(P.hcounts[b].get()[i], 0), cap);
            yolo2_hip_det *dst = dets + (size_t)f * cap;
            memcpy(dst, P.hdets[b].get() + (size_t)i * cap, (size_t)cnt * sizeof(yolo2_hip_det));
            for (int r = 0; r < cnt; ++r) dst[r].frame = f;   // frame numbers are global in the caller's records
            const int *hi = L.hinfo[b].get() + 2 * i;
            if (drawn) drawn[f] = hi[0];
            info.items_built += (uint64_t)hi[0];
            if (hi[1] && bad_frame < 0) bad_frame = f;
            if (jpeg) {
                const size_t size = (size_t)J.hsizes[b].get()[i], bytes = std::min(size, caps[f]);
                if (bytes) memcpy(out[f], J.hout[b].get() + off, bytes);
                off += bytes;
                sizes[f] = size;
                if (size > caps[f] && short_frame < 0) short_frame = f;
            } else {
                const size_t bytes = (size_t)widths[f] * heights[f] * 3;
                memcpy(out[f], A.hout[b].get() + off, bytes);
                off += padded(bytes);
                sizes[f] = bytes;
            }
        }
        return YOLO2_SUCCESS;
    };

    std::vector<size_t> offs((size_t)batch), out_offs((size_t)batch), fbytes((size_t)batch);
    std::vector<int> cw((size_t)batch), chh((size_t)batch);
    std::vector<hipEvent_t> wait_for;   // what the tail of a chunk waits for
    for (int k = 0; k < chunks; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        // (buffer set b is free: chunk k - 2 was delivered in the round before - ordering (1) above)
        uint8_t *hin = P.hin[b].get();
        size_t off = lead, out_off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i;
            fbytes[(size_t)i] = (size_t)widths[f] * heights[f] * ch;
            offs[(size_t)i] = off;
            out_offs[(size_t)i] = out_off;
            jf[(size_t)i] = {widths[f], heights[f], out_off, caps[f]};
            off += padded(fbytes[(size_t)i]);
            out_off += padded((size_t)widths[f] * heights[f] * 3);
            info.image_bytes_staged += fbytes[(size_t)i];
        }
        y2_stage_images(hin, images + first, offs.data(), fbytes.data(), nf);   // the frames, once
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(hin);
        for (int f = 0; f < batch; ++f) {   // a partial last chunk repeats its last image
            const int i = std::min(f, nf - 1);
            cw[(size_t)f] = widths[first + i]; chh[(size_t)f] = heights[first + i];
            items[f].off = offs[(size_t)i];
            if ((rc = y2_letterbox_args(widths[first + i], heights[first + i], ch, 416, 416, items[f].a, true))) { cleanup(); return rc; }
        }
        const int max_strips = y2_loop_fill_geom(hin + lb_bytes, nf, cw.data(), chh.data(), ch, offs.data(), out_offs.data());
        const size_t jtab = off;
        if (jpeg) {
            y2_jpeg_write_table(jf.data(), nf, quality, hin + jtab);
            off += plans[(size_t)k].table_bytes;
        }
        if ((rc = y2_post_fill_geom(P.hgeom[b].get(), cw.data(), chh.data(), batch))) { cleanup(); return rc; }
        Y2_TRY(hipMemcpyAsync(P.dbytes[b].get(), hin, off, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);   // the one upload
        Y2_TRY(hipMemcpyAsync(P.post[b].geom.get(), P.hgeom[b].get(), (size_t)batch * gbytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_in[b], P.s_in), YOLO2_ERROR);
        info.image_bytes_h2d += off;
        ++info.chunks;
        Y2_TRY(hipStreamWaitEvent(P.s_run, P.e_in[b], 0), YOLO2_ERROR);
        // ---- the network, by the code the _pix_dets entry of the precision runs it with
        if (i16) {
            rc = y2_pipe_enqueue_i16(c, b, yuyv, batch, &q, &wait_for);
        } else {
            rc = y2_pipe_enqueue_f16(c, run, fused, b, yuyv, batch);
            wait_for.assign(1, P.e_run[b]);
        }
        if (rc) { cleanup(); return rc; }
        // ---- the chunk before: its stream bytes go onto s_out ahead of the wait for this chunk's network (ordering (3))
        if (jpeg && k >= 1 && (rc = fetch(k - 1))) return rc;
        for (hipEvent_t e : wait_for) Y2_TRY(hipStreamWaitEvent(P.s_out, e, 0), YOLO2_ERROR);
        // ---- tail, draw items, painter, encoder: all on s_out
        if (i16) rc = y2_post_enqueue_int16(c->device, P.dout[b].get(), batch, q, thresh, nms, cap, 1, app_tail, &P.post[b], P.s_out);
        else rc = y2_post_enqueue_f32(P.dregf[b].get(), batch, thresh, nms, cap, 1, app_tail, &P.post[b], P.s_out);
        if (rc) { cleanup(); return rc; }
        Y2_TRY(hipMemcpyAsync(P.hcounts[b].get(), P.post[b].counts.get(), (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipMemcpyAsync(P.hdets[b].get(), P.post[b].dets.get(), (size_t)batch * cap * sizeof(yolo2_hip_det), hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        if ((rc = y2_loop_enqueue_items(c, b, nf, cap, thresh, labels, n_labels, P.dbytes[b].get() + lb_bytes, P.post[b].dets.get(), P.post[b].counts.get(),
                                        P.s_out)) ||
            (rc = y2_loop_enqueue_paint(c, nf, max_strips, P.dbytes[b].get(), jpeg ? J.rgb.get() : A.dout[b].get(), P.s_out))) {
            cleanup();
            return rc;
        }
        if (jpeg) {
            const Y2JpegPlan &plan = plans[(size_t)k];
            if ((rc = y2_jpeg_enqueue(plan, P.dbytes[b].get() + jtab, J.rgb.get(), J.work.get(), J.dout[b].get(), P.s_out))) { cleanup(); return rc; }
            Y2_TRY(hipMemcpyAsync(J.hsizes[b].get(), J.work.get() + plan.sizes, (size_t)nf * sizeof(unsigned long long), hipMemcpyDeviceToHost, P.s_out),
                   YOLO2_DMA_ERROR);
            Y2_TRY(hipEventRecord(J.e_sizes[b], P.s_out), YOLO2_ERROR);
        } else {
            Y2_TRY(hipMemcpyAsync(A.hout[b].get(), A.dout[b].get(), out_off, hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
            Y2_TRY(hipEventRecord(P.e_out[b], P.s_out), YOLO2_ERROR);
            info.out_bytes_d2h += out_off;
        }
        if (k >= 1 && (rc = deliver(k - 1))) return rc;
    }
    if (jpeg && (rc = fetch(chunks - 1))) return rc;
    if ((rc = deliver(chunks - 1))) return rc;
#undef Y2_TRY
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    if (i16 && final_q) *final_q = q;
    if (!i16) c->images_l0[split] = fused ? std::string(y2_f16_images_kernel(run, yuyv))
                                          : std::string(yuyv ? "k_letterbox_yuyv_batch + " : "k_letterbox_u8_batch + ") + yolo2_hip_fp16_layer_kernel(run, 0);
    c->loop_info = info;
    if (bad_frame >= 0)
        return fail(YOLO2_ERROR, "loop: frame %d has a record with a non-finite (or 2^23 and larger) prob among those to be drawn", bad_frame);
    if (short_frame >= 0)
        return fail(YOLO2_ERROR, "loop: output buffer too small for frame %d (%zu < %zu bytes)", short_frame, caps[short_frame], sizes[short_frame]);
    return YOLO2_SUCCESS;
}
