// yolo2_loop.hip -- the camera loop as one call (include/yolo2_hip.h, "the camera loop as one call"): frames -> detection records AND
// the annotated frames (RGB24, BGR24, planar YUV 4:2:0 as NV12 / I420, or JPEG) from ONE upload per chunk.
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
//
// From JPEG streams (yolo2_hip_loop_images_jpeg): the same loop with the decoder stage of yolo2_jpegdec.hip (y2_jpegdec.hpp) in front of
// the network.  The staging buffer keeps its layout, but a frame that arrives as a stream is not staged: its slot in dbytes[b] is
// written by k_jpegdec_rgb (k_jpegdec_zero for a flagged scan), and the front kernel, the painter and the encoder read it there.
//   s_in    the chunk's blob (descriptors, tables, streams) -> djpg[b]; tables in front of the slots, the caller's raw frames each
//           into its slot, and with JPEG out the encoder's table behind the slots -> dbytes[b]
//   s_run   coefficient memset, entropy stage (option jpegdec_split: two launches), k_jpegdec_idct, _rgb, _zero; then the network
//   s_out   as above, with the decoder's status words copied out behind the records
// (1) holds unchanged and now also covers the decoder: it WRITES the slots of dbytes[b] on s_run, and chunk k + 2 is staged and its
// decoder enqueued only after deliver(k), so the painter of chunk k (s_out) has read them; djpg[b] and the pinned blob follow the same
// rule (the status words of chunk k are copied out on s_out in front of e_out[b]).  (2) gains one line: the decoder's coefficient
// and plane buffers exist once and are touched by kernels of s_run only, the stream that keeps the chunks' decoders and networks in
// order (the int16 lanes' streams never see them).  (3) is unchanged.  A frame the decoder flags is painted and encoded like any
// other (zero pixels), but nothing of it is handed out: status[f] != 0, counts[f] = drawn[f] = 0, sizes[f] = 0, out[f] untouched.
#include "y2_internal.hpp"
#include "letterbox.hpp"
#include "y2_draw.hpp"
#include "y2_jpeg.hpp"
#include "y2_jpegdec.hpp"

using namespace y2;

namespace {
size_t padded(size_t b) { return (b + 255) & ~(size_t)255; }
bool out_yuv420(int out_format) { return out_format == YOLO2_LOOP_OUT_NV12 || out_format == YOLO2_LOOP_OUT_I420; }
// bytes of a painted frame on the device: planar 4:2:0 (w, h even), or packed RGB24 / BGR24 (also what the JPEG route paints for its encoder)
size_t out_frame_bytes(int out_format, int w, int h) { return out_yuv420(out_format) ? (size_t)w * h * 3 / 2 : (size_t)w * h * 3; }
}  // namespace

// (y2_draw.hpp) everything the loop entries refuse that can be seen without a context
int y2_loop_check(int precision, const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch, float thresh,
                  int flags, const yolo2_hip_det *dets, int cap_per_frame, const int *counts, int n_labels, int out_format, int quality,
                  uint8_t *const *out, const size_t *caps, const size_t *sizes)
{
    if (!images || !widths || !heights || !dets || !counts || !out || !caps || !sizes) return fail(YOLO2_ERROR, "loop: null argument");
    if (precision != YOLO2_LOOP_INT16 && precision != YOLO2_LOOP_FP16 && precision != YOLO2_LOOP_F32TOL)
        return fail(YOLO2_ERROR, "loop: unknown precision %d (YOLO2_LOOP_INT16, _FP16 or _F32TOL)", precision);
    if (out_format != YOLO2_LOOP_OUT_RGB24 && out_format != YOLO2_LOOP_OUT_JPEG && out_format != YOLO2_LOOP_OUT_BGR24 && !out_yuv420(out_format))
        return fail(YOLO2_ERROR, "loop: unknown output format %d (YOLO2_LOOP_OUT_RGB24, _JPEG, _BGR24, _NV12 or _I420)", out_format);
    if (!(flags & YOLO2_DETS_BEST_CLASS)) return fail(YOLO2_ERROR, "loop: flags must contain YOLO2_DETS_BEST_CLASS, the form the painter draws");
    const Y2PixDesc *pd = y2_pix_desc(pixfmt, nullptr);
    if (!pd) return YOLO2_ERROR;
    const int ch = pd->ch;
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
        } else {
            if (out_yuv420(out_format) && ((widths[f] | heights[f]) & 1))
                return fail(YOLO2_ERROR, "loop: frame %d is %dx%d: YUV 4:2:0 output needs an even width and height (odd sizes are refused)", f, widths[f],
                            heights[f]);
            const size_t need = out_frame_bytes(out_format, widths[f], heights[f]);
            if (caps[f] < need) return fail(YOLO2_ERROR, "loop: output buffer too small for frame %d (%zu < %zu bytes)", f, caps[f], need);
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

// The chunk loop of both loop entries.  dec == nullptr: images are frames of pixfmt, staged and uploaded whole.  Otherwise: images are
// the streams (and raw RGB24 frames) the decoder stage dec has the headers of, and status [n] receives its words.
static int loop_run(yolo2_hip_ctx *c, int precision, const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch,
                    float thresh, float nms, int flags, yolo2_hip_det *dets, int cap, int *counts, int *final_q, const char *const *labels, int n_labels,
                    int out_format, int quality, uint8_t *const *out, const size_t *caps, size_t *sizes, int *drawn, Y2JpegDec *dec, int *status,
                    const size_t *stream_bytes)
{
    int rc;
    const bool i16 = precision == YOLO2_LOOP_INT16, jpeg = out_format == YOLO2_LOOP_OUT_JPEG;
    const int split = precision == YOLO2_LOOP_F32TOL ? 1 : 0, ch = y2_pix_desc(pixfmt, nullptr)->ch, app_tail = (flags & YOLO2_DETS_APP_TAIL) ? 1 : 0;
    const int kind = y2_ch_kind(ch);
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
            in += padded(y2_frame_bytes(widths[f], heights[f], ch));
            jf[(size_t)i] = {widths[f], heights[f], rgb, caps[f]};
            rgb += padded(out_frame_bytes(out_format, widths[f], heights[f]));
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
    if (dec && (rc = y2_jpegdec_plan(dec, batch))) return rc;
    if (i16 && batch != c->batch && (rc = yolo2_hip_set_batch(c, batch))) return rc;
    if ((rc = y2_pipe_ensure(c->pipe, cap_in, cap_in, batch, false)) || (rc = y2_pipe_ensure_post(c, batch, cap))) return rc;
    if (dec && (rc = y2_jpegdec_ensure(dec))) return rc;     // (behind y2_pipe_ensure: growing that drops the decoder's buffers)
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

    int short_frame = -1, bad_frame = -1, flagged_frame = -1, q = 0;
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
        if (dec) y2_jpegdec_collect(dec, k, status, &flagged_frame);
        size_t off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i, cnt = std::min(std::max(P.hcounts[b].get()[i], 0), cap);
            if (dec && status[f]) {   // a flagged scan: nothing of the frame is handed out; its bytes in the packed output are stepped over
                counts[f] = 0;
                if (drawn) drawn[f] = 0;
                sizes[f] = 0;
                off += jpeg ? std::min((size_t)J.hsizes[b].get()[i], caps[f]) : padded(out_frame_bytes(out_format, widths[f], heights[f]));
                continue;
            }
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
                const size_t bytes = out_frame_bytes(out_format, widths[f], heights[f]);
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
    double up_tables = 0;               // (streams) bytes uploaded into dbytes[b] beside the raw frames
    for (int k = 0; k < chunks; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        // (buffer set b is free: chunk k - 2 was delivered in the round before - ordering (1) above)
        uint8_t *hin = P.hin[b].get();
        size_t off = lead, out_off = 0;
        for (int i = 0; i < nf; ++i) {
            const int f = first + i;
            fbytes[(size_t)i] = y2_frame_bytes(widths[f], heights[f], ch);
            offs[(size_t)i] = off;
            out_offs[(size_t)i] = out_off;
            jf[(size_t)i] = {widths[f], heights[f], out_off, caps[f]};
            off += padded(fbytes[(size_t)i]);
            out_off += padded(out_frame_bytes(out_format, widths[f], heights[f]));
            info.image_bytes_staged += dec && !y2_jpegdec_raw(dec, f) ? stream_bytes[f] : fbytes[(size_t)i];
        }
        if (!dec) y2_stage_images(hin, images + first, offs.data(), fbytes.data(), nf);   // the frames, once
        else if ((rc = y2_jpegdec_stage(dec, k, offs.data(), hin))) { cleanup(); return rc; }   // the blob (uploaded) and the raw frames
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(hin);
        for (int f = 0; f < batch; ++f) {   // a partial last chunk repeats its last image
            const int i = std::min(f, nf - 1);
            cw[(size_t)f] = widths[first + i]; chh[(size_t)f] = heights[first + i];
            items[f].off = offs[(size_t)i];
            if ((rc = y2_letterbox_args(widths[first + i], heights[first + i], ch, 416, 416, items[f].a, true))) { cleanup(); return rc; }
        }
        const int max_strips = y2_loop_fill_geom(hin + lb_bytes, nf, cw.data(), chh.data(), ch, offs.data(), out_offs.data(), out_format);
        const size_t jtab = off;
        if (jpeg) {
            y2_jpeg_write_table(jf.data(), nf, quality, hin + jtab);
            off += plans[(size_t)k].table_bytes;
        }
        if ((rc = y2_post_fill_geom(P.hgeom[b].get(), cw.data(), chh.data(), batch))) { cleanup(); return rc; }
        if (!dec) {
            Y2_TRY(hipMemcpyAsync(P.dbytes[b].get(), hin, off, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);   // the one upload
            info.image_bytes_h2d += off;
        } else {   // the tables around the slots and the raw frames; the slots of the streams are the decoder's to write
            Y2_TRY(hipMemcpyAsync(P.dbytes[b].get(), hin, lead, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
            if ((rc = y2_jpegdec_upload_raw(dec, k, offs.data(), hin))) { cleanup(); return rc; }
            if (off > jtab) Y2_TRY(hipMemcpyAsync(P.dbytes[b].get() + jtab, hin + jtab, off - jtab, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
            up_tables += (double)(lead + (off - jtab));
        }
        Y2_TRY(hipMemcpyAsync(P.post[b].geom.get(), P.hgeom[b].get(), (size_t)batch * gbytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_in[b], P.s_in), YOLO2_ERROR);
        ++info.chunks;
        Y2_TRY(hipStreamWaitEvent(P.s_run, P.e_in[b], 0), YOLO2_ERROR);
        if (dec && (rc = y2_jpegdec_launch(dec, k))) { cleanup(); return rc; }   // ---- the decoder, into the slots
        // ---- the network, by the code the _pix_dets entry of the precision runs it with
        if (i16) {
            rc = y2_pipe_enqueue_i16(c, b, kind, batch, &q, &wait_for);
        } else {
            rc = y2_pipe_enqueue_f16(c, run, fused, b, kind, batch);
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
        if (dec && (rc = y2_jpegdec_status_d2h(dec, k, P.s_out))) { cleanup(); return rc; }
        if ((rc = y2_loop_enqueue_items(c, b, nf, cap, thresh, labels, n_labels, P.dbytes[b].get() + lb_bytes, P.post[b].dets.get(), P.post[b].counts.get(),
                                        P.s_out)) ||
            (rc = y2_loop_enqueue_paint(c, nf, max_strips, P.dbytes[b].get(), jpeg ? J.rgb.get() : A.dout[b].get(), jpeg ? YOLO2_LOOP_OUT_RGB24 : out_format, P.s_out))) {
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
    if (!i16) c->images_l0[split] = fused ? std::string(y2_f16_images_kernel(run, kind))
                                          : std::string(y2_letterbox_batch_kernel(kind)) + " + " + yolo2_hip_fp16_layer_kernel(run, 0);
    if (dec) {
        info.image_bytes_h2d = (uint64_t)(y2_jpegdec_uploaded(dec) + up_tables);
        y2_jpegdec_close(dec, up_tables);
    }
    c->loop_info = info;
    if (flagged_frame >= 0)
        return fail(YOLO2_ERROR, "loop: frame %d: the GPU decoder flagged its scan (status %d); nothing of it is returned, decode it on the host",
                    flagged_frame, status[flagged_frame]);
    if (bad_frame >= 0)
        return fail(YOLO2_ERROR, "loop: frame %d has a record with a non-finite (or 2^23 and larger) prob among those to be drawn", bad_frame);
    if (short_frame >= 0)
        return fail(YOLO2_ERROR, "loop: output buffer too small for frame %d (%zu < %zu bytes)", short_frame, caps[short_frame], sizes[short_frame]);
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
    return loop_run(c, precision, images, widths, heights, pixfmt, n, batch, thresh, nms, flags, dets, cap, counts, final_q, labels, n_labels, out_format,
                    quality, out, caps, sizes, drawn, nullptr, nullptr, nullptr);
}

// Everything the loop entry from streams refuses that can be seen without a device: the probe's refusals, then - on the sizes the
// headers give, left in wh (widths, then heights) - y2_loop_check's.  Touches none of the caller's arrays.  c == nullptr: the check
// alone (the multi entry, before it starts a shard).
static int loop_jpeg_open(yolo2_hip_ctx *c, int precision, const uint8_t *const *streams, const size_t *stream_sizes, const int *widths,
                          const int *heights, int n, int batch, float thresh, int flags, const yolo2_hip_det *dets, int cap, const int *counts,
                          int n_labels, int out_format, int quality, uint8_t *const *out, const size_t *caps, const size_t *sizes, const int *status,
                          std::vector<int> &wh, Y2JpegDecPtr *dec)
{
    if (!streams || !stream_sizes || !widths || !heights || !status) return fail(YOLO2_ERROR, "loop: null argument");
    if (precision == YOLO2_JPEG_INT8) return fail(YOLO2_ERROR, "loop: the loop entries have no int8 form (YOLO2_LOOP_INT16, _FP16 or _F32TOL)");
    if (n <= 0 || batch <= 0 || batch > 1024 || cap <= 0 || cap > 65536)
        return fail(YOLO2_ERROR, "loop: bad image count %d / batch %d (1..1024) / capacity %d (1..65536)", n, batch, cap);
    wh.assign(widths, widths + n);
    wh.insert(wh.end(), heights, heights + n);
    int rc;
    if ((rc = y2_jpegdec_open(c, streams, stream_sizes, wh.data(), wh.data() + n, n, true, nullptr, dec))) return rc;
    return y2_loop_check(precision, streams, wh.data(), wh.data() + n, YOLO2_PIX_RGB24, n, batch, thresh, flags, dets, cap, counts, n_labels, out_format,
                         quality, out, caps, sizes);
}

// (y2_draw.hpp)
int y2_loop_jpeg_check(int precision, const uint8_t *const *streams, const size_t *stream_sizes, const int *widths, const int *heights, int n, int batch,
                       float thresh, int flags, const yolo2_hip_det *dets, int cap, const int *counts, int n_labels, int out_format, int quality,
                       uint8_t *const *out, const size_t *caps, const size_t *sizes, const int *status)
{
    std::vector<int> wh;
    Y2JpegDecPtr dec;
    return loop_jpeg_open(nullptr, precision, streams, stream_sizes, widths, heights, n, batch, thresh, flags, dets, cap, counts, n_labels, out_format,
                          quality, out, caps, sizes, status, wh, &dec);
}

extern "C" int yolo2_hip_loop_images_jpeg(yolo2_hip_ctx *c, int precision, const uint8_t *const *streams, const size_t *stream_sizes, int *widths,
                                          int *heights, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap,
                                          int *counts, int *final_q, const char *const *labels, int n_labels, int out_format, int quality,
                                          uint8_t *const *out, const size_t *caps, size_t *sizes, int *drawn, int *status)
{
    if (!c) return fail(YOLO2_ERROR, "loop: null argument");
    std::vector<int> wh;
    Y2JpegDecPtr dec;
    int rc;
    if ((rc = loop_jpeg_open(c, precision, streams, stream_sizes, widths, heights, n, batch, thresh, flags, dets, cap, counts, n_labels, out_format,
                             quality, out, caps, sizes, status, wh, &dec)))
        return rc;
    // (the network's own refusals: loop_run's, here in front of the first write to the caller's arrays)
    if (precision == YOLO2_LOOP_INT16 ? !c->weights_loaded : (!c->f16_loaded || !c->f16_plan || !c->wf32))
        return fail(YOLO2_ERROR, precision == YOLO2_LOOP_INT16 ? "loop: int16 weights not loaded" : "loop: fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    memcpy(widths, wh.data(), (size_t)n * sizeof(int));
    memcpy(heights, wh.data() + n, (size_t)n * sizeof(int));
    return loop_run(c, precision, streams, widths, heights, YOLO2_PIX_RGB24, n, batch, thresh, nms, flags, dets, cap, counts, final_q, labels, n_labels,
                    out_format, quality, out, caps, sizes, drawn, dec.get(), status, stream_sizes);
}
