// yolo2_jpegdec.hip -- JPEG streams -> RGB24 / detection records with the decoder on the GPU (include/yolo2_hip.h, "JPEG streams
// decoded on the GPU").  The probe and the host doorway (jpeg_parse.hpp over jpeg_scan.hpp), the launches of
// kernels_jpegdec.hpp as a stage of a chunk loop (y2_jpegdec.hpp; the loop entry from streams, yolo2_loop.hip, calls it too), and
// the one chunk loop behind the two GPU entries.
//
// A chunk, in buffer set b of PipeBufs:
//   host    headers parsed; hjpg[b] = the blob (Frame[], Segment[], the workgroups' table sets, status words, Tables[] - identical
//           sets once - and the streams, each on a 16-byte boundary); hin[b] = the LetterboxItem table and the caller's raw frames at
//           their slots, exactly the staging layout of run_images_regf
//   s_in    blob -> djpg[b] (the one upload of the compressed route); table and raw frames -> dbytes[b]
//   s_run   memset of the coefficients, k_jpegdec_entropy (under option jpegdec_split: k_jpegdec_split, then k_jpegdec_rest - their
//           tables SplitSeg[] / SplitWg[] lie in the blob in front of the streams, a word per segment behind the status words), _idct, _rgb (into the frames' slots of dbytes[b]), _zero; then the
//           network of the precision by the code its _pix_dets entry runs it with, reading dbytes[b] as if the host had filled it
//   s_out   tail + D2H of records, counts and status words (records entry), or D2H of the slots and status words (decode entry)
// Buffer set b is refilled for chunk k + 2 after drain(k) has waited for e_out[b]; the coefficient and plane buffers exist once and
// are touched on s_run only, which keeps chunks in order.
#include "y2_internal.hpp"
#include "letterbox.hpp"
#include "jpeg_parse.hpp"
#include "kernels_jpegdec.hpp"
#include "y2_jpegdec.hpp"

using namespace y2;
using namespace y2jpg;

namespace {
size_t padded(size_t b) { return (b + 255) & ~(size_t)255; }
const char *kReasonNames[] = {"accepted", "damaged or unsupported header", "progressive", "unsupported SOF type or sample precision",
                              "4 components", "RGB colour space", "sampling factors", "not exactly one interleaved scan followed by EOI",
                              "missing Huffman table", "too large"};
}  // namespace

extern "C" const char *yolo2_hip_jpeg_reason_name(int reason)
{
    return reason >= 0 && reason < (int)(sizeof(kReasonNames) / sizeof(kReasonNames[0])) ? kReasonNames[reason] : "unknown";
}

extern "C" int yolo2_hip_jpeg_probe(const uint8_t *jpeg, size_t size, yolo2_hip_jpeg_info_t *info)
{
    if (!jpeg || !info) return fail(YOLO2_ERROR, "null argument");
    Info i;
    parse(jpeg, size, i, nullptr);
    info->width = i.width; info->height = i.height; info->components = i.components; info->hmax = i.hmax; info->vmax = i.vmax;
    info->restart_interval = i.restart_interval; info->gpu_decodable = i.gpu_decodable; info->reason = i.reason;
    info->stream_bytes = i.stream_bytes;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_decode_jpeg_ref(const uint8_t *stream, size_t size, uint8_t *rgb_out, size_t cap, int *width, int *height, int *status)
{
    if (!stream || !rgb_out || !status) return fail(YOLO2_ERROR, "null argument");
    int w = 0, h = 0;
    *status = 0;
    const int why = decode_ref(stream, size, rgb_out, cap, &w, &h, status);
    if (width) *width = w;
    if (height) *height = h;
    if (why > 0) {
        *status = 100 + why;
        return fail(YOLO2_ERROR, "not GPU-decodable: %s", yolo2_hip_jpeg_reason_name(why));
    }
    if (why < 0) return fail(YOLO2_ERROR, "output buffer too small (%zu < %zu bytes)", cap, (size_t)w * h * 3);
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_decode_jpeg_split_ref(const uint8_t *stream, size_t size, int split_bytes, uint8_t *rgb_out, size_t cap, int *width, int *height,
                                               int *status, double *info8)
{
    if (!stream || !rgb_out || !status || !info8) return fail(YOLO2_ERROR, "null argument");
    if (split_bytes < kSplitMin || split_bytes > kSplitMax || split_bytes % 16)
        return fail(YOLO2_ERROR, "split_bytes %d: a multiple of 16 in %d..%d", split_bytes, kSplitMin, kSplitMax);
    int w = 0, h = 0;
    *status = 0;
    const int why = decode_ref(stream, size, rgb_out, cap, &w, &h, status, split_bytes, info8);
    if (width) *width = w;
    if (height) *height = h;
    if (why > 0) {
        *status = 100 + why;
        return fail(YOLO2_ERROR, "not GPU-decodable: %s", yolo2_hip_jpeg_reason_name(why));
    }
    if (why < 0) return fail(YOLO2_ERROR, "output buffer too small (%zu < %zu bytes)", cap, (size_t)w * h * 3);
    return YOLO2_SUCCESS;
}

namespace {

int jpeg_ensure(PipeBufs &P, size_t blob, size_t samples, size_t status_words)
{
    if (P.jpg_blob < blob) {
        P.jpg_blob = 0;
        for (int k = 0; k < 2; ++k) {
            int rc;
            if ((rc = P.hjpg[k].alloc(blob)) || (rc = P.djpg[k].alloc(blob))) return rc;
        }
        P.jpg_blob = blob;
    }
    if (P.jpg_samples < samples) {
        P.jpg_samples = 0;
        int rc;
        if ((rc = P.jcoef.alloc(samples)) || (rc = P.jplanes.alloc(samples))) return rc;
        P.jpg_samples = samples;
    }
    if (P.jpg_status < status_words) {
        P.jpg_status = 0;
        for (int k = 0; k < 2; ++k) {
            const int rc = P.hjstatus[k].alloc(status_words);
            if (rc) return rc;
        }
        P.jpg_status = status_words;
    }
    return YOLO2_SUCCESS;
}

struct ChunkLayout {
    uint32_t segs_off, wg_off, status_off, tables_off, streams_off;
    uint32_t sseg_off, swg_off;    // option jpegdec_split: SplitSeg[], SplitWg[]; the segments' words follow the status words
    int n_seg, n_wg, n_swg;
    // what the launches of the chunk need beside the offsets
    size_t words, coef_off;
    int max_blocks;
    unsigned max_pixels;
};

}  // namespace

// ---------------------------------------------------------------------------- the decoder as a stage (y2_jpegdec.hpp)

struct Y2JpegDec {
    yolo2_hip_ctx *c = nullptr;
    const uint8_t *const *streams = nullptr;
    const size_t *sizes = nullptr;
    const int *widths = nullptr, *heights = nullptr;
    int n = 0, batch = 0, chunks = 0;
    int split = 0;                       // option jpegdec_split as read when the call began; 0: today's launches exactly
    std::vector<Parsed> parsed;
    size_t cap_blob = 0, cap_samples = 0, cap_status = 0;
    ChunkLayout lay[2] = {};
    double split_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double up_blob = 0, up_raw = 0;
    // under yolo2_hip_set_profiling: five timing events per chunk around the memset and the three kernels (yolo2_hip_jpeg_last_info);
    // with the option a sixth, behind the first chunks * 5: between k_jpegdec_split and k_jpegdec_rest
    std::vector<hipEvent_t> prof;
    int in_chunk(int k) const { return std::min(batch, n - k * batch); }
    ~Y2JpegDec() { for (hipEvent_t x : prof) (void)hipEventDestroy(x); }
};

void Y2JpegDecDelete::operator()(Y2JpegDec *d) const { delete d; }

int y2_jpegdec_open(yolo2_hip_ctx *c, const uint8_t *const *streams, const size_t *sizes, int *widths, int *heights, int n, bool raw_ok,
                    const std::function<int(int)> &check, Y2JpegDecPtr *out)
{
    Y2JpegDecPtr d(new Y2JpegDec());
    d->c = c; d->streams = streams; d->sizes = sizes; d->widths = widths; d->heights = heights; d->n = n;
    d->split = c ? c->opt.jpegdec_split : 0;      // read per call (no context: the headers are all the caller wants)
    d->split_info[5] = (double)d->split;
    d->parsed.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!streams[i]) return fail(YOLO2_ERROR, "frame %d: null stream", i);
        Parsed &p = d->parsed[(size_t)i];
        if (sizes[i] == 0) {
            if (!raw_ok) return fail(YOLO2_ERROR, "frame %d: empty stream", i);
            memset(&p.f, 0, sizeof(p.f));
            p.f.raw = 1; p.f.width = widths[i]; p.f.height = heights[i];
        } else {
            Info info;
            if (parse(streams[i], sizes[i], info, &p))
                return fail(YOLO2_ERROR, "frame %d: not GPU-decodable (reason %d: %s)", i, info.reason, yolo2_hip_jpeg_reason_name(info.reason));
            widths[i] = info.width; heights[i] = info.height;
        }
        const int rc = check ? check(i) : YOLO2_SUCCESS;
        if (rc) return rc;
    }
    *out = std::move(d);
    return YOLO2_SUCCESS;
}

bool y2_jpegdec_raw(const Y2JpegDec *d, int frame) { return d->parsed[(size_t)frame].f.raw != 0; }

int y2_jpegdec_plan(Y2JpegDec *d, int batch)
{
    d->batch = batch;
    d->chunks = (d->n + batch - 1) / batch;
    const int split = d->split;
    for (int k = 0; k < d->chunks; ++k) {
        size_t str = 0, samples = 0, segs = 0;
        for (int i = k * batch; i < k * batch + d->in_chunk(k); ++i) {
            str += (d->sizes[i] + 15) & ~(size_t)15;
            samples += d->parsed[(size_t)i].f.samples;
            segs += d->parsed[(size_t)i].segs.size();
        }
        const size_t nf = (size_t)d->in_chunk(k), wgs = (segs + kEntropyLanes - 1) / kEntropyLanes;
        // (jpegdec_split: at most one SplitSeg and one SplitWg per segment, and a word per segment behind the status words)
        const size_t words = nf + segs * (split ? 2 : 1);
        const size_t blob = padded(nf * sizeof(Frame)) + padded(segs * sizeof(Segment)) + padded(wgs * sizeof(int)) + padded(words * sizeof(int)) +
                            padded(nf * sizeof(Tables)) + padded(str) + (split ? padded(segs * sizeof(SplitSeg)) + padded(segs * sizeof(SplitWg)) : 0);
        if (blob > (size_t)1 << 31) return fail(YOLO2_ERROR, "chunk %d: more than 2 GiB of streams and tables (use a smaller batch)", k);
        d->cap_blob = std::max(d->cap_blob, blob); d->cap_samples = std::max(d->cap_samples, samples);
        d->cap_status = std::max(d->cap_status, words);
    }
    return YOLO2_SUCCESS;
}

int y2_jpegdec_ensure(Y2JpegDec *d)
{
    int rc;
    if ((rc = jpeg_ensure(d->c->pipe, d->cap_blob, std::max<size_t>(d->cap_samples, 64), d->cap_status))) return rc;
    if (d->c->prof)
        for (int i = 0; i < d->chunks * (d->split ? 6 : 5); ++i) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e), YOLO2_ERROR);
            d->prof.push_back(e);
        }
    return YOLO2_SUCCESS;
}

int y2_jpegdec_stage(Y2JpegDec *d, int k, const size_t *slot, uint8_t *hin)
{
    PipeBufs &P = d->c->pipe;
    const int b = k & 1, nf = d->in_chunk(k), first = k * d->batch, split = d->split;
    const std::vector<Parsed> &parsed = d->parsed;
    uint8_t *blob = P.hjpg[b].get();
    // ---- blob layout
    int n_seg = 0;
    for (int f = 0; f < nf; ++f) n_seg += (int)parsed[(size_t)(first + f)].segs.size();
    ChunkLayout &L = d->lay[b];
    L.n_seg = n_seg; L.n_wg = (n_seg + kEntropyLanes - 1) / kEntropyLanes;
    L.segs_off = (uint32_t)padded((size_t)nf * sizeof(Frame));
    L.wg_off = L.segs_off + (uint32_t)padded((size_t)n_seg * sizeof(Segment));
    L.status_off = L.wg_off + (uint32_t)padded((size_t)L.n_wg * sizeof(int));
    const size_t words = (size_t)nf + (size_t)n_seg * (split ? 2 : 1);
    L.words = words;
    L.tables_off = L.status_off + (uint32_t)padded(words * sizeof(int));
    Frame *frames = reinterpret_cast<Frame *>(blob);
    Segment *segs = reinterpret_cast<Segment *>(blob + L.segs_off);
    int *wg = reinterpret_cast<int *>(blob + L.wg_off), *st = reinterpret_cast<int *>(blob + L.status_off);
    Tables *tables = reinterpret_cast<Tables *>(blob + L.tables_off);
    memset(st, 0, words * sizeof(int));
    // ---- table sets: identical ones once
    int n_sets = 0;
    std::vector<int> set_of((size_t)nf, 0);
    for (int f = 0; f < nf; ++f) {
        const Parsed &p = parsed[(size_t)(first + f)];
        if (p.f.raw) continue;
        int s = 0;
        while (s < n_sets && memcmp(tables + s, &p.t, sizeof(Tables)) != 0) ++s;
        if (s == n_sets) memcpy(tables + n_sets++, &p.t, sizeof(Tables));
        set_of[(size_t)f] = s;
    }
    L.sseg_off = L.tables_off + (uint32_t)padded((size_t)n_sets * sizeof(Tables));
    L.swg_off = L.sseg_off + (split ? (uint32_t)padded((size_t)n_seg * sizeof(SplitSeg)) : 0u);
    L.streams_off = L.swg_off + (split ? (uint32_t)padded((size_t)n_seg * sizeof(SplitWg)) : 0u);
    L.n_swg = 0;
    // ---- frames, segments, streams; the RGB24 slots
    size_t at = L.streams_off, coef_off = 0;
    int seg = 0, max_blocks = 0;
    unsigned max_pixels = 0;
    for (int f = 0; f < nf; ++f) {
        const Parsed &p = parsed[(size_t)(first + f)];
        const int i = first + f;
        Frame &F = frames[f];
        F = p.f;
        F.tables = set_of[(size_t)f];
        F.first_seg = seg; F.n_seg = (int)p.segs.size();
        F.coef_off = F.plane_off = coef_off;
        F.rgb_off = slot[f];
        const size_t bytes = (size_t)d->widths[i] * d->heights[i] * 3;
        if (p.f.raw) {
            memcpy(hin + slot[f], d->streams[i], bytes);
        } else {
            st[f] = p.status;
            memcpy(blob + at, d->streams[i], d->sizes[i]);
            for (const Segment &s : p.segs) {
                Segment &ds = segs[seg++];
                ds = s;
                ds.begin += (uint32_t)at; ds.end += (uint32_t)at; ds.frame = f;
            }
            at += (d->sizes[i] + 15) & ~(size_t)15;
            coef_off += p.f.samples;
            max_blocks = std::max(max_blocks, p.f.blocks);
            max_pixels = std::max(max_pixels, (unsigned)d->widths[i] * (unsigned)d->heights[i]);
        }
    }
    L.coef_off = coef_off; L.max_blocks = max_blocks; L.max_pixels = max_pixels;
    const size_t blob_bytes = padded(at);
    memset(blob + at, 0, blob_bytes - at);
    for (int w = 0; w < L.n_wg; ++w) {
        const int lo = w * kEntropyLanes, hi = std::min(n_seg, lo + kEntropyLanes), s0 = frames[segs[lo].frame].tables;
        bool same = true;
        for (int j = lo + 1; j < hi && same; ++j) same = frames[segs[j].frame].tables == s0;
        wg[w] = same ? s0 : -1;
    }
    if (split) {
        // the workgroups of k_jpegdec_split: consecutive segments of one frame, at least two subsequences each, filled up to
        // kSplitMaxSub subsequences / kSplitWgSegs segments
        SplitSeg *sseg = reinterpret_cast<SplitSeg *>(blob + L.sseg_off);
        SplitWg *swg = reinterpret_cast<SplitWg *>(blob + L.swg_off);
        int n_ss = 0;
        for (int f = 0; f < nf; ++f) {
            SplitWg cur = {n_ss, 0, 0, 0};
            for (int j = frames[f].first_seg; j < frames[f].first_seg + (frames[f].raw ? 0 : frames[f].n_seg); ++j) {
                const SplitPlan sp = split_plan(blob, segs[j], split);
                if (sp.n_sub < 2) { d->split_info[3] += 1; continue; }
                if (cur.n == kSplitWgSegs || cur.n_tasks + sp.n_sub > kSplitMaxSub) {
                    swg[L.n_swg++] = cur;
                    cur = SplitWg{n_ss, 0, 0, 0};
                }
                sseg[n_ss++] = SplitSeg{sp.data_end, j, sp.sub, sp.n_sub, cur.n_tasks, {0, 0, 0}};
                ++cur.n; cur.n_tasks += sp.n_sub; cur.rounds = std::max(cur.rounds, sp.n_sub - 1);
                d->split_info[0] += sp.n_sub;
            }
            if (cur.n) swg[L.n_swg++] = cur;
        }
    }
    HIP_TRY(hipMemcpyAsync(P.djpg[b].get(), blob, blob_bytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
    d->up_blob += (double)blob_bytes;
    return YOLO2_SUCCESS;
}

int y2_jpegdec_upload_raw(Y2JpegDec *d, int k, const size_t *slot, const uint8_t *hin)
{
    PipeBufs &P = d->c->pipe;
    const int b = k & 1, nf = d->in_chunk(k), first = k * d->batch;
    for (int f = 0; f < nf; ++f)
        if (d->parsed[(size_t)(first + f)].f.raw) {
            const size_t bytes = (size_t)d->widths[first + f] * d->heights[first + f] * 3;
            HIP_TRY(hipMemcpyAsync(P.dbytes[b].get() + slot[f], hin + slot[f], bytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
            d->up_raw += (double)bytes;
        }
    return YOLO2_SUCCESS;
}

int y2_jpegdec_launch(Y2JpegDec *d, int k)
{
    PipeBufs &P = d->c->pipe;
    const int b = k & 1, nf = d->in_chunk(k), chunks = d->chunks;
    const ChunkLayout &L = d->lay[b];
    auto stamp = [&](int i) { if (!d->prof.empty()) (void)hipEventRecord(d->prof[(size_t)(k * 5 + i)], P.s_run); };
    JpegDecArgs a;
    a.blob = P.djpg[b].get();
    a.frames_off = 0; a.segs_off = L.segs_off; a.wg_off = L.wg_off; a.status_off = L.status_off; a.tables_off = L.tables_off;
    a.n_frames = nf; a.n_seg = L.n_seg;
    a.coef = P.jcoef.get(); a.planes = P.jplanes.get(); a.rgb = P.dbytes[b].get();
    stamp(0);
    if (L.coef_off) HIP_TRY(hipMemsetAsync(P.jcoef.get(), 0, L.coef_off * sizeof(int16_t), P.s_run), YOLO2_ERROR);
    stamp(1);
    if (d->split && L.n_seg) {
        JpegSplitArgs sa;
        sa.seg_off = L.sseg_off; sa.wg_off = L.swg_off; sa.word_off = L.status_off + (uint32_t)((size_t)(nf + L.n_seg) * sizeof(int));
        if (L.n_swg) hipLaunchKernelGGL(k_jpegdec_split, dim3((unsigned)L.n_swg), dim3(kSplitThreads), 0, P.s_run, a, sa);
        if (!d->prof.empty()) (void)hipEventRecord(d->prof[(size_t)(chunks * 5 + k)], P.s_run);
        hipLaunchKernelGGL(k_jpegdec_rest, dim3((unsigned)L.n_wg), dim3(kEntropyLanes), 0, P.s_run, a, sa);
    } else if (L.n_seg) {
        hipLaunchKernelGGL(k_jpegdec_entropy, dim3((unsigned)L.n_wg), dim3(kEntropyLanes), 0, P.s_run, a);
    }
    stamp(2);
    if (L.max_blocks) hipLaunchKernelGGL(k_jpegdec_idct, dim3(blocks_for(L.max_blocks, kIdctThreads), (unsigned)nf), dim3(kIdctThreads), 0, P.s_run, a);
    stamp(3);
    if (L.max_blocks) hipLaunchKernelGGL(k_jpegdec_rgb, dim3(blocks_for((long)L.max_pixels, kRgbThreads), (unsigned)nf), dim3(kRgbThreads), 0, P.s_run, a);
    if (L.max_pixels) hipLaunchKernelGGL(k_jpegdec_zero, dim3(64, (unsigned)nf), dim3(256), 0, P.s_run, a);
    stamp(4);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

int y2_jpegdec_status_d2h(Y2JpegDec *d, int k, hipStream_t st)
{
    PipeBufs &P = d->c->pipe;
    const int b = k & 1;
    HIP_TRY(hipMemcpyAsync(P.hjstatus[b].get(), P.djpg[b].get() + d->lay[b].status_off, d->lay[b].words * sizeof(int), hipMemcpyDeviceToHost, st),
            YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

void y2_jpegdec_collect(Y2JpegDec *d, int k, int *status, int *first_bad)
{
    const int b = k & 1, nf = d->in_chunk(k), first = k * d->batch;
    const int *st = d->c->pipe.hjstatus[b].get();
    int n_seg = 0, seg = 0;
    for (int f = 0; f < nf; ++f) n_seg += (int)d->parsed[(size_t)(first + f)].segs.size();
    if (d->split)
        for (int j = 0; j < n_seg; ++j) {
            const unsigned word = (unsigned)st[nf + n_seg + j];
            if (!word) continue;
            d->split_info[(word & 1u) ? 1 : 2] += 1;
            d->split_info[4] = std::max(d->split_info[4], (double)(word >> 2));
        }
    for (int f = 0; f < nf; ++f) {
        const Parsed &p = d->parsed[(size_t)(first + f)];
        int s = st[f];
        for (size_t j = 0; j < p.segs.size() && !s; ++j) s = st[nf + seg + (int)j];      // the first failing interval in stream order
        seg += (int)p.segs.size();
        status[first + f] = s;
        if (s && *first_bad < 0) *first_bad = first + f;
    }
}

double y2_jpegdec_uploaded(const Y2JpegDec *d) { return d->up_blob + d->up_raw; }

void y2_jpegdec_close(Y2JpegDec *d, double other_bytes)
{
    const int chunks = d->chunks;
    double *info = d->c->jpeg_dec_info;
    for (int i = 0; i < 8; ++i) info[i] = 0;
    for (int k = 0; k < chunks && !d->prof.empty(); ++k)
        for (int i = 0; i < 4; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, d->prof[(size_t)(k * 5 + i)], d->prof[(size_t)(k * 5 + i + 1)]) == hipSuccess) info[i] += ms / chunks;
        }
    info[4] = d->up_blob; info[5] = other_bytes + d->up_raw; info[6] = chunks; info[7] = d->n;
    for (int k = 0; k < chunks && d->split && !d->prof.empty(); ++k) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, d->prof[(size_t)(k * 5 + 1)], d->prof[(size_t)(chunks * 5 + k)]) == hipSuccess) d->split_info[6] += ms / chunks;
        if (hipEventElapsedTime(&ms, d->prof[(size_t)(chunks * 5 + k)], d->prof[(size_t)(k * 5 + 2)]) == hipSuccess) d->split_info[7] += ms / chunks;
    }
    memcpy(d->c->jpeg_split_info, d->split_info, sizeof(d->split_info));
}

namespace {

// dets == nullptr: the decode entry (rgb_out / caps); otherwise the records entry
int run_jpeg(yolo2_hip_ctx *c, int precision, const uint8_t *const *streams, const size_t *sizes, int *widths, int *heights, int n, int batch,
             uint8_t *const *rgb_out, const size_t *caps, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap, int *counts, int *final_q,
             int *status)
{
    const bool want_dets = dets != nullptr;
    if (!c || !streams || !sizes || !widths || !heights || !status || (want_dets ? !counts : (!rgb_out || !caps))) return fail(YOLO2_ERROR, "null argument");
    if (n <= 0 || batch <= 0 || batch > 1024 || (want_dets && cap <= 0))
        return fail(YOLO2_ERROR, "bad image count %d / batch %d (1..1024) / capacity %d", n, batch, want_dets ? cap : 1);
    if (want_dets && thresh < 0.f) return fail(YOLO2_ERROR, "negative threshold");
    const bool i16 = precision == YOLO2_LOOP_INT16, i8 = precision == YOLO2_JPEG_INT8;
    if (want_dets && !i16 && !i8 && precision != YOLO2_LOOP_FP16 && precision != YOLO2_LOOP_F32TOL)
        return fail(YOLO2_ERROR, "unknown precision %d (YOLO2_LOOP_INT16, _FP16, _F32TOL or YOLO2_JPEG_INT8)", precision);
    // ---- headers: every refusal before anything is launched
    Y2JpegDecPtr dec;
    int rc;
    if ((rc = y2_jpegdec_open(c, streams, sizes, widths, heights, n, want_dets, [&](int i) -> int {
            if (sizes[i] && !want_dets) {
                if (caps[i] < (size_t)widths[i] * heights[i] * 3)
                    return fail(YOLO2_ERROR, "frame %d: output buffer too small (%zu < %zu bytes)", i, caps[i], (size_t)widths[i] * heights[i] * 3);
                if (!rgb_out[i]) return fail(YOLO2_ERROR, "frame %d: null output", i);
            }
            if (want_dets) {
                LetterboxArgs a;
                return y2_letterbox_args(widths[i], heights[i], 3, 416, 416, a, true);
            }
            return YOLO2_SUCCESS;
        }, &dec)))
        return rc;
    // ---- the network's own refusals
    yolo2_hip_ctx *run = nullptr;
    bool fused = false;
    if (want_dets) {
        if (i16) {
            if (!c->weights_loaded) return fail(YOLO2_ERROR, "weights not loaded");
        } else if (i8) {
            if (!y2_i8_loaded(c)) return fail(YOLO2_ERROR, "int8 weights not loaded (yolo2_hip_load_weights_int8)");
            fused = y2_i8_images_fused(c);
        } else {
            if ((rc = y2_f16_images_ctx(c, precision == YOLO2_LOOP_F32TOL ? 1 : 0, &run))) return rc;
            fused = y2_f16_images_fused(run);
        }
    }
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch, best_only = (flags & YOLO2_DETS_BEST_CLASS) ? 1 : 0, app_tail = (flags & YOLO2_DETS_APP_TAIL) ? 1 : 0;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    const size_t table_bytes = padded((size_t)batch * sizeof(LetterboxItem));
    // ---- sizes of the largest chunk
    size_t cap_rgb = 0;
    for (int k = 0; k < chunks; ++k) {
        size_t rgb = table_bytes;
        for (int i = k * batch; i < k * batch + in_chunk(k); ++i) rgb += padded((size_t)widths[i] * heights[i] * 3);
        cap_rgb = std::max(cap_rgb, rgb);
    }
    if ((rc = y2_jpegdec_plan(dec.get(), batch))) return rc;
    if (want_dets && i16 && batch != c->batch && (rc = yolo2_hip_set_batch(c, batch))) return rc;
    if ((rc = y2_pipe_ensure(c->pipe, cap_rgb, cap_rgb, batch, false))) return rc;     // (first: growing it drops every other buffer of PipeBufs)
    if (want_dets && !i16 && (rc = y2_pipe_ensure_regf(c->pipe, batch, false))) return rc;
    if (want_dets && (rc = y2_pipe_ensure_post(c, batch, cap))) return rc;
    PipeBufs &P = c->pipe;
    const size_t gbytes = y2_post_geom_bytes();
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)
    if ((rc = y2_jpegdec_ensure(dec.get()))) { cleanup(); return rc; }

    std::vector<std::vector<size_t>> slot(2, std::vector<size_t>((size_t)batch));
    int first_bad = -1;
    auto drain = [&](int k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        (void)hipEventSynchronize(P.e_out[b]);
        y2_jpegdec_collect(dec.get(), k, status, &first_bad);
        for (int f = 0; f < nf; ++f) {
            const int s = status[first + f];
            if (!want_dets) {
                const size_t bytes = (size_t)widths[first + f] * heights[first + f] * 3;
                memcpy(rgb_out[first + f], P.hin[b].get() + slot[(size_t)b][(size_t)f], bytes);
                continue;
            }
            const int cnt = s ? 0 : std::min(P.hcounts[b].get()[f], cap);
            counts[first + f] = s ? 0 : P.hcounts[b].get()[f];
            yolo2_hip_det *dst = dets + (size_t)(first + f) * cap;
            memcpy(dst, P.hdets[b].get() + (size_t)f * cap, (size_t)cnt * sizeof(yolo2_hip_det));
            for (int r = 0; r < cnt; ++r) dst[r].frame = first + f;
        }
    };
    int q = 0;
    std::vector<int> cw((size_t)batch), chh((size_t)batch);
    std::vector<hipEvent_t> net_done;
    double up_tables = 0;
    for (int k = 0; k < chunks; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        if (k >= 2) drain(k - 2);
        uint8_t *hin = P.hin[b].get();
        // ---- the RGB24 slots behind the letterbox table, then the blob (and its upload)
        size_t rgb_off = table_bytes;
        for (int f = 0; f < nf; ++f) {
            slot[(size_t)b][(size_t)f] = rgb_off;
            rgb_off += padded((size_t)widths[first + f] * heights[first + f] * 3);
        }
        if ((rc = y2_jpegdec_stage(dec.get(), k, slot[(size_t)b].data(), hin))) { cleanup(); return rc; }
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(hin);
        for (int f = 0; f < batch; ++f) {   // a partial last chunk repeats its last image
            const int i = std::min(f, nf - 1);
            cw[(size_t)f] = widths[first + i]; chh[(size_t)f] = heights[first + i];
            items[f].off = slot[(size_t)b][(size_t)i];
            if ((rc = y2_letterbox_args(widths[first + i], heights[first + i], 3, 416, 416, items[f].a, true))) { cleanup(); return rc; }
        }
        if (want_dets && (rc = y2_post_fill_geom(P.hgeom[b].get(), cw.data(), chh.data(), batch))) { cleanup(); return rc; }
        // ---- the other uploads
        Y2_TRY(hipMemcpyAsync(P.dbytes[b].get(), hin, table_bytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        if ((rc = y2_jpegdec_upload_raw(dec.get(), k, slot[(size_t)b].data(), hin))) { cleanup(); return rc; }
        if (want_dets) Y2_TRY(hipMemcpyAsync(P.post[b].geom.get(), P.hgeom[b].get(), (size_t)batch * gbytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_in[b], P.s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(P.s_run, P.e_in[b], 0), YOLO2_ERROR);
        up_tables += (double)table_bytes;
        // ---- the decoder
        if ((rc = y2_jpegdec_launch(dec.get(), k))) { cleanup(); return rc; }
        // ---- behind it
        if (!want_dets) {
            Y2_TRY(hipEventRecord(P.e_run[b], P.s_run), YOLO2_ERROR);
            Y2_TRY(hipStreamWaitEvent(P.s_out, P.e_run[b], 0), YOLO2_ERROR);
            Y2_TRY(hipMemcpyAsync(hin + table_bytes, P.dbytes[b].get() + table_bytes, rgb_off - table_bytes, hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        } else {
            if (i16) {
                rc = y2_pipe_enqueue_i16(c, b, false, batch, &q, &net_done);
            } else if (i8) {
                if (fused) {
                    rc = y2_i8_run_images(c, P.dbytes[b].get(), false, batch, P.dregf[b].get(), P.s_run);
                } else {
                    y2_launch_letterbox_batch(false, P.dbytes[b].get(), P.din[b].get(), batch, P.s_run);
                    rc = yolo2_hip_run_batch_int8(c, (uint64_t)(uintptr_t)P.din[b].get(), batch, (uint64_t)(uintptr_t)P.dregf[b].get(), P.s_run);
                }
                if (rc == YOLO2_SUCCESS) Y2_TRY(hipEventRecord(P.e_run[b], P.s_run), YOLO2_ERROR);
                net_done.assign(1, P.e_run[b]);
            } else {
                rc = y2_pipe_enqueue_f16(c, run, fused, b, false, batch);
                net_done.assign(1, P.e_run[b]);
            }
            if (rc) { cleanup(); return rc; }
            for (hipEvent_t e : net_done) Y2_TRY(hipStreamWaitEvent(P.s_out, e, 0), YOLO2_ERROR);
            if (i16) rc = y2_post_enqueue_int16(c->device, P.dout[b].get(), batch, q, thresh, nms, cap, best_only, app_tail, &P.post[b], P.s_out);
            else rc = y2_post_enqueue_f32(P.dregf[b].get(), batch, thresh, nms, cap, best_only, app_tail, &P.post[b], P.s_out);
            if (rc) { cleanup(); return rc; }
            Y2_TRY(hipMemcpyAsync(P.hcounts[b].get(), P.post[b].counts.get(), (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
            Y2_TRY(hipMemcpyAsync(P.hdets[b].get(), P.post[b].dets.get(), (size_t)batch * cap * sizeof(yolo2_hip_det), hipMemcpyDeviceToHost, P.s_out),
                   YOLO2_DMA_ERROR);
        }
        if ((rc = y2_jpegdec_status_d2h(dec.get(), k, P.s_out))) { cleanup(); return rc; }
        Y2_TRY(hipEventRecord(P.e_out[b], P.s_out), YOLO2_ERROR);
    }
    for (int k = std::max(0, chunks - 2); k < chunks; ++k) drain(k);
    cleanup();
#undef Y2_TRY
    y2_jpegdec_close(dec.get(), up_tables);
    if (want_dets && i16 && final_q) *final_q = q;
    if (first_bad >= 0)
        return fail(YOLO2_ERROR, "frame %d: the GPU decoder flagged its scan (status %d); it is zero-filled, decode it on the host", first_bad, status[first_bad]);
    return YOLO2_SUCCESS;
}

}  // namespace

extern "C" int yolo2_hip_jpeg_last_info(yolo2_hip_ctx *c, double *out8)
{
    if (!c || !out8) return fail(YOLO2_ERROR, "null argument");
    memcpy(out8, c->jpeg_dec_info, sizeof(c->jpeg_dec_info));
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_jpeg_split_info(yolo2_hip_ctx *c, double *out8)
{
    if (!c || !out8) return fail(YOLO2_ERROR, "null argument");
    memcpy(out8, c->jpeg_split_info, sizeof(c->jpeg_split_info));
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_decode_jpeg_host(yolo2_hip_ctx *c, const uint8_t *const *streams, const size_t *sizes, int n, int batch,
                                          uint8_t *const *rgb_out, const size_t *caps, int *widths, int *heights, int *status)
{
    return run_jpeg(c, -1, streams, sizes, widths, heights, n, batch, rgb_out, caps, 0.f, 0.f, 0, nullptr, 0, nullptr, nullptr, status);
}

extern "C" int yolo2_hip_run_images_jpeg_dets(yolo2_hip_ctx *c, int precision, const uint8_t *const *streams, const size_t *sizes, int *widths,
                                              int *heights, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                              int cap_per_frame, int *counts, int *final_q, int *status)
{
    if (!dets) return fail(YOLO2_ERROR, "null argument");
    return run_jpeg(c, precision, streams, sizes, widths, heights, n, batch, nullptr, nullptr, thresh, nms, flags, dets, cap_per_frame, counts, final_q,
                    status);
}
