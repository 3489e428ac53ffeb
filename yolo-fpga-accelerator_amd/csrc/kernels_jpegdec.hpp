// kernels_jpegdec.hpp -- baseline JPEG streams in device memory -> RGB24 frames in the chunk staging layout the images entries read.
// Included by yolo2_jpegdec.hip only.  The arithmetic is jpeg_scan.hpp's (shared with the host doorway); this file is the mapping of
// that work onto the machine:
//   k_jpegdec_entropy   one lane per restart interval: Huffman decode + dequantisation into the frame's coefficient blocks.  Scalar-like
//                       work on a vector machine: the lanes of a wavefront walk different streams, so every memory access is a gather and
//                       the loops run as long as the slowest lane.  Bounded by the geometry (MCUs x blocks x 64 turns), never the data.
//   k_jpegdec_split     option jpegdec_split: one lane per subsequence of a segment, a workgroup per group of segments; speculate,
//                       synchronise, scan, accept, write.  k_jpegdec_rest: k_jpegdec_entropy for the segments it did not take.
//   k_jpegdec_idct      one thread per 8x8 block: 128 bytes of coefficients in, 64 samples out, the block in registers.
//   k_jpegdec_rgb       one thread per output pixel: up-sample + YCbCr -> RGB24 (or the grey sample three times).
//   k_jpegdec_zero      a frame whose status is not 0: its RGB24 slot zero-filled before anything reads it.
// The chunk's blob (one H2D) holds, at the offsets in JpegDecArgs: Frame[n_frames], Segment[n_seg], the table set of every workgroup of
// the entropy kernel (-1: its lanes name different sets), the status words (frames, then segments), Tables[], then the streams.
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_scan.hpp"

namespace y2jpg {

struct JpegDecArgs {
    const uint8_t *blob;           // 256-byte aligned; Segment::begin / end are offsets into it
    uint32_t frames_off, segs_off, wg_off, status_off, tables_off;
    int n_frames, n_seg;
    int16_t *coef;                 // zeroed in front of the entropy kernel
    uint8_t *planes;
    uint8_t *rgb;                  // the chunk's device staging buffer; Frame::rgb_off is relative to it
};

constexpr int kEntropyLanes = 64;  // one wavefront per workgroup: a table set in LDS (9.1 KB) serves 64 segments

__global__ __launch_bounds__(kEntropyLanes) void k_jpegdec_entropy(JpegDecArgs a)
{
    __shared__ uint4 lds_tables[sizeof(Tables) / 16];
    const Frame *frames = reinterpret_cast<const Frame *>(a.blob + a.frames_off);
    const Segment *segs = reinterpret_cast<const Segment *>(a.blob + a.segs_off);
    const Tables *tables = reinterpret_cast<const Tables *>(a.blob + a.tables_off);
    const int wg_set = reinterpret_cast<const int *>(a.blob + a.wg_off)[blockIdx.x];
    if (wg_set >= 0) {             // (uniform) every lane of this workgroup reads the same set: from LDS
        const uint4 *src = reinterpret_cast<const uint4 *>(tables + wg_set);
        for (unsigned i = threadIdx.x; i < sizeof(Tables) / 16; i += kEntropyLanes) lds_tables[i] = src[i];
        __syncthreads();
    }
    const int i = (int)(blockIdx.x * kEntropyLanes + threadIdx.x);
    if (i >= a.n_seg) return;
    const Segment s = segs[i];
    const Frame &f = frames[s.frame];
    const Tables *t = wg_set >= 0 ? reinterpret_cast<const Tables *>(lds_tables) : tables + f.tables;
    const int st = decode_segment(f, *t, a.blob, s, a.coef + f.coef_off);
    if (st) reinterpret_cast<int *>(const_cast<uint8_t *>(a.blob) + a.status_off)[a.n_frames + i] = st;   // the lane's own word
}

// ---- option jpegdec_split: many lanes per segment (jpeg_scan.hpp "one segment, many lanes")
// The host's tables, in the blob: SplitSeg[] - the segments of at least two subsequences - and SplitWg[], one entry per workgroup of
// k_jpegdec_split: consecutive split segments of ONE frame (so one table set, in LDS) with at most kSplitMaxSub subsequences and
// kSplitWgSegs segments between them.  A subsequence is a "task"; the workgroup's threads loop over its tasks.  A segment never spans
// workgroups, so every hand-off is a __syncthreads().  The word of a segment behind the status words (split_off): 0 - not split (its
// lane of k_jpegdec_rest decodes it), otherwise rounds << 2 | 1 (accepted: its coefficients are written) or | 2 (fell back).
struct SplitSeg {
    uint32_t data_end;
    int seg, sub, n_sub, first_task;    // first_task: of its subsequence 0 among the workgroup's tasks
    int pad[3];
};
struct SplitWg {
    int first, n, n_tasks, rounds;      // SplitSeg[first .. first + n); rounds: most (n_sub - 1) of them
};
struct JpegSplitArgs {
    uint32_t seg_off, wg_off, word_off; // SplitSeg[], SplitWg[], the segments' words
};
constexpr int kSplitThreads = 1024, kSplitWgSegs = 256, kSplitChunk = kSplitMaxSub / kSplitThreads;
static_assert(kSplitMaxSub % kSplitThreads == 0 && kSplitWgSegs <= kSplitThreads, "the scan gives each thread kSplitChunk consecutive tasks");

// Records, running states and prefixes live in LDS as one array per field (a lane's words are 4 bytes apart from its neighbour's).
struct SplitLds {
    uint32_t off[kSplitMaxSub], meta[kSplitMaxSub], nblk[kSplitMaxSub];
    int32_t dc[3][kSplitMaxSub];
    uint32_t cur_off[kSplitMaxSub], cur_meta[kSplitMaxSub];     // a lane's own exit state between rounds; kSplitDone: it has stopped looking
    uint32_t pre_nblk[kSplitMaxSub];                            // exclusive prefix of nblk (dc[] is scanned in place; stopped-before: kSplitBefore in meta)
    uint16_t task_seg[kSplitMaxSub];
    uint32_t agg[kSplitThreads][6];                             // a thread's chunk: starts a segment, then blocks, DC sums, stopped
    uint32_t seg_closes[kSplitWgSegs], seg_over[kSplitWgSegs], seg_rounds[kSplitWgSegs];   // a lane closes it / overshoots; rounds used
};
constexpr uint32_t kSplitDone = 1u << 14, kSplitBefore = 1u << 15;

__device__ inline SplitRec split_load(const SplitLds &L, int q)
{
    SplitRec r;
    r.off = L.off[q]; r.meta = L.meta[q]; r.nblk = L.nblk[q]; r.dc[0] = L.dc[0][q]; r.dc[1] = L.dc[1][q]; r.dc[2] = L.dc[2][q];
    return r;
}
__device__ inline void split_store(SplitLds &L, int q, const SplitRec &r)
{
    L.off[q] = r.off; L.meta[q] = r.meta; L.nblk[q] = r.nblk; L.dc[0][q] = r.dc[0]; L.dc[1][q] = r.dc[1]; L.dc[2][q] = r.dc[2];
}

// grid: the chunk's SplitWg entries.  Every thread reaches every barrier: the task loops are skipped, never the barriers behind them;
// the round loop's exit is __syncthreads_or's.  Trip counts: tasks and rounds from the host's table, symbols 8 * sub + 16.
__global__ __launch_bounds__(kSplitThreads) void k_jpegdec_split(JpegDecArgs a, JpegSplitArgs sa)
{
    __shared__ uint4 lds_tables[sizeof(Tables) / 16];
    __shared__ SplitLds L;
    const Frame *frames = reinterpret_cast<const Frame *>(a.blob + a.frames_off);
    const Segment *segs = reinterpret_cast<const Segment *>(a.blob + a.segs_off);
    const SplitSeg *ss = reinterpret_cast<const SplitSeg *>(a.blob + sa.seg_off);
    const SplitWg wg = reinterpret_cast<const SplitWg *>(a.blob + sa.wg_off)[blockIdx.x];
    const int tid = (int)threadIdx.x;
    ss += wg.first;
    const Frame &f = frames[segs[ss[0].seg].frame];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const Tables *>(a.blob + a.tables_off) + f.tables);
        for (unsigned i = threadIdx.x; i < sizeof(Tables) / 16; i += kSplitThreads) lds_tables[i] = src[i];
    }
    const Tables &t = *reinterpret_cast<const Tables *>(lds_tables);
    for (int j = tid; j < wg.n; j += kSplitThreads) {
        const SplitSeg e = ss[j];
        for (int u = 0; u < e.n_sub; ++u) L.task_seg[e.first_task + u] = (uint16_t)j;
        L.seg_closes[j] = 0; L.seg_over[j] = 0; L.seg_rounds[j] = 0;
    }
    __syncthreads();
    int bpm = 0;
    const uint32_t smap = split_slot_map(f, bpm);
    SplitWrite none = {};
    // what a task's lane needs to decode subsequence q (q: task index; the same segment's)
    auto sub_end = [&](const SplitSeg &e, uint32_t begin, int u) {
        const unsigned long long x = (unsigned long long)begin + (unsigned long long)(u + 1) * (unsigned)e.sub;
        return x < e.data_end ? (uint32_t)x : e.data_end;
    };
    // ---- 1. speculate
    for (int q = tid; q < wg.n_tasks; q += kSplitThreads) {
        const SplitSeg e = ss[L.task_seg[q]];
        const uint32_t begin = segs[e.seg].begin;
        const int u = q - e.first_task;
        SplitRec r;
        split_run<false>(f, t, a.blob, e.data_end, sub_end(e, begin, u), smap, bpm, 8 * e.sub + 16, begin + (uint32_t)u * (uint32_t)e.sub, 0u, r, none);
        split_store(L, q, r);
        L.cur_off[q] = r.off;
        L.cur_meta[q] = (r.meta & kSplitStateMask) | ((r.meta & kSplitStopped) ? kSplitDone : 0u);
    }
    __syncthreads();
    // ---- 2. synchronise: in round r the lane of task q decodes subsequence q + r + 1 of its segment from its own exit state; nobody
    // else reads or writes that record in the round
    for (int r = 0; r < wg.rounds; ++r) {
        int any = 0;
        for (int q = tid; q < wg.n_tasks; q += kSplitThreads) {
            const uint32_t cm = L.cur_meta[q];
            if (cm & kSplitDone) continue;
            const int j = L.task_seg[q];
            const SplitSeg e = ss[j];
            const int u = q - e.first_task + r + 1;
            if (u >= e.n_sub) { L.cur_meta[q] = cm | kSplitDone; continue; }
            SplitRec out;
            split_run<false>(f, t, a.blob, e.data_end, sub_end(e, segs[e.seg].begin, u), smap, bpm, 8 * e.sub + 16, L.cur_off[q], cm & kSplitStateMask, out, none);
            L.seg_rounds[j] = (uint32_t)(r + 1);                 // (every writer of the round stores the same value)
            if (split_same(out, split_load(L, q + r + 1))) { L.cur_meta[q] = cm | kSplitDone; continue; }
            split_store(L, q + r + 1, out);
            L.cur_off[q] = out.off;
            if (out.meta & kSplitStopped) L.cur_meta[q] = cm | kSplitDone;
            else { L.cur_meta[q] = out.meta & kSplitStateMask; any = 1; }
        }
        if (!__syncthreads_or(any)) break;
    }
    __syncthreads();
    // ---- 3. scan, segmented at the segments' first tasks: a thread's kSplitChunk consecutive tasks, then the chunks' carries by one
    // thread, then the chunk again with its carry
    const int q0 = tid * kSplitChunk;
    auto chunk = [&](bool store, uint32_t run[5]) {
        bool starts = false;
        for (int i = 0; i < kSplitChunk; ++i) {
            const int q = q0 + i;
            if (q >= wg.n_tasks) break;
            if (ss[L.task_seg[q]].first_task == q) { starts = true; run[0] = run[1] = run[2] = run[3] = run[4] = 0; }
            const uint32_t n = L.nblk[q], m = L.meta[q], d0 = (uint32_t)L.dc[0][q], d1 = (uint32_t)L.dc[1][q], d2 = (uint32_t)L.dc[2][q];
            if (store) {
                L.pre_nblk[q] = run[0]; L.dc[0][q] = (int32_t)run[1]; L.dc[1][q] = (int32_t)run[2]; L.dc[2][q] = (int32_t)run[3];
                L.meta[q] = m | (run[4] ? kSplitBefore : 0u);
            }
            run[0] += n; run[1] += d0; run[2] += d1; run[3] += d2; run[4] |= m & kSplitStopped;
        }
        return starts;
    };
    {
        uint32_t run[5] = {0, 0, 0, 0, 0};
        L.agg[tid][5] = chunk(false, run) ? 1u : 0u;
        for (int i = 0; i < 5; ++i) L.agg[tid][i] = run[i];
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t carry[5] = {0, 0, 0, 0, 0};
        const int chunks = (wg.n_tasks + kSplitChunk - 1) / kSplitChunk;
        for (int c = 0; c < chunks; ++c) {
            for (int i = 0; i < 5; ++i) {
                const uint32_t own = L.agg[c][i];
                L.agg[c][i] = carry[i];
                carry[i] = L.agg[c][5] ? own : (i == 4 ? carry[i] | own : carry[i] + own);
            }
        }
    }
    __syncthreads();
    {
        uint32_t run[5];
        for (int i = 0; i < 5; ++i) run[i] = L.agg[tid][i];
        chunk(true, run);
    }
    __syncthreads();
    // ---- 4. accept
    for (int q = tid; q < wg.n_tasks; q += kSplitThreads) {
        const int j = L.task_seg[q];
        const uint32_t n_blocks = (uint32_t)segs[ss[j].seg].n_mcu * (uint32_t)bpm;
        SplitRec own;
        own.meta = L.meta[q]; own.nblk = L.nblk[q];
        const bool before = (own.meta & kSplitBefore) != 0;
        if (split_closes(L.pre_nblk[q], before, own, n_blocks)) L.seg_closes[j] = 1u;       // (plain stores of one value)
        if (split_overshoots(L.pre_nblk[q], before, own, n_blocks)) L.seg_over[j] = 1u;
    }
    __syncthreads();
    // ---- 5. write: the lanes of accepted segments once more, from the verified state, into the frame's coefficients
    for (int q = tid; q < wg.n_tasks; q += kSplitThreads) {
        const int j = L.task_seg[q];
        if (!L.seg_closes[j] || L.seg_over[j]) continue;
        const SplitSeg e = ss[j];
        const Segment s = segs[e.seg];
        const uint32_t n_blocks = (uint32_t)s.n_mcu * (uint32_t)bpm, m = L.meta[q];
        if ((m & kSplitBefore) || L.pre_nblk[q] >= n_blocks) continue;
        const int u = q - e.first_task;
        SplitWrite w = {(int)L.pre_nblk[q], (int)n_blocks, s.first_mcu, {L.dc[0][q], L.dc[1][q], L.dc[2][q]}, a.coef + f.coef_off};
        SplitRec out;
        split_run<true>(f, t, a.blob, e.data_end, sub_end(e, s.begin, u), smap, bpm, 8 * e.sub + 16, u ? L.off[q - 1] : s.begin,
                        u ? L.meta[q - 1] & kSplitStateMask : 0u, out, w);
    }
    for (int j = tid; j < wg.n; j += kSplitThreads)
        reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(a.blob) + sa.word_off)[ss[j].seg] = (L.seg_rounds[j] << 2) | (L.seg_closes[j] && !L.seg_over[j] ? 1u : 2u);
}

// k_jpegdec_entropy for what k_jpegdec_split left: the lanes of segments it accepted return at once (behind the barrier); every other
// segment - too short to split, or fallen back, with its coefficients still zero - is decode_segment's, and the status word is that
// function's.
__global__ __launch_bounds__(kEntropyLanes) void k_jpegdec_rest(JpegDecArgs a, JpegSplitArgs sa)
{
    __shared__ uint4 lds_tables[sizeof(Tables) / 16];
    const Frame *frames = reinterpret_cast<const Frame *>(a.blob + a.frames_off);
    const Segment *segs = reinterpret_cast<const Segment *>(a.blob + a.segs_off);
    const Tables *tables = reinterpret_cast<const Tables *>(a.blob + a.tables_off);
    const int wg_set = reinterpret_cast<const int *>(a.blob + a.wg_off)[blockIdx.x];
    if (wg_set >= 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(tables + wg_set);
        for (unsigned i = threadIdx.x; i < sizeof(Tables) / 16; i += kEntropyLanes) lds_tables[i] = src[i];
        __syncthreads();
    }
    const int i = (int)(blockIdx.x * kEntropyLanes + threadIdx.x);
    if (i >= a.n_seg) return;
    if (reinterpret_cast<const uint32_t *>(a.blob + sa.word_off)[i] & 1u) return;
    const Segment s = segs[i];
    const Frame &f = frames[s.frame];
    const Tables *t = wg_set >= 0 ? reinterpret_cast<const Tables *>(lds_tables) : tables + f.tables;
    const int st = decode_segment(f, *t, a.blob, s, a.coef + f.coef_off);
    if (st) reinterpret_cast<int *>(const_cast<uint8_t *>(a.blob) + a.status_off)[a.n_frames + i] = st;
}

constexpr int kIdctThreads = 64;

// grid (ceil(most blocks of a frame / 64), n_frames)
__global__ __launch_bounds__(kIdctThreads) void k_jpegdec_idct(JpegDecArgs a)
{
    const Frame &f = reinterpret_cast<const Frame *>(a.blob + a.frames_off)[blockIdx.y];
    const int j = (int)(blockIdx.x * kIdctThreads + threadIdx.x);
    if (j >= f.blocks) return;
    int k = 0;
    if (f.ncomp == 3) k = (uint32_t)j * 64u >= f.comp[2].off ? 2 : ((uint32_t)j * 64u >= f.comp[1].off ? 1 : 0);
    const Comp &c = f.comp[k];
    const int local = j - (int)(c.off / 64u), bw = c.w2 >> 3, bx = local % bw, by = local / bw;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.coef + f.coef_off + (size_t)j * 64);   // (coef_off is a multiple of 64)
    int16_t d[64];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 w = src[q];
        d[q * 8 + 0] = (int16_t)(w.x & 0xffffu); d[q * 8 + 1] = (int16_t)(w.x >> 16);
        d[q * 8 + 2] = (int16_t)(w.y & 0xffffu); d[q * 8 + 3] = (int16_t)(w.y >> 16);
        d[q * 8 + 4] = (int16_t)(w.z & 0xffffu); d[q * 8 + 5] = (int16_t)(w.z >> 16);
        d[q * 8 + 6] = (int16_t)(w.w & 0xffffu); d[q * 8 + 7] = (int16_t)(w.w >> 16);
    }
    idct_block(a.planes + f.plane_off + c.off + (size_t)by * 8 * c.w2 + (size_t)bx * 8, c.w2, d);
}

constexpr int kRgbThreads = 256;

// grid (ceil(most pixels of a frame / 256), n_frames)
__global__ __launch_bounds__(kRgbThreads) void k_jpegdec_rgb(JpegDecArgs a)
{
    const Frame &f = reinterpret_cast<const Frame *>(a.blob + a.frames_off)[blockIdx.y];
    if (f.raw) return;
    const unsigned p = blockIdx.x * kRgbThreads + threadIdx.x;
    if (p >= (unsigned)f.width * (unsigned)f.height) return;
    const int y = (int)(p / (unsigned)f.width), x = (int)(p - (unsigned)y * (unsigned)f.width);
    uint8_t px[3];
    rgb_pixel(f, a.planes + f.plane_off, x, y, px);
    uint8_t *out = a.rgb + f.rgb_off + (size_t)p * 3;
    out[0] = px[0]; out[1] = px[1]; out[2] = px[2];
}

// grid (blocks, n_frames): the frame's status words (its own, then its segments') reduced by every workgroup; a flagged frame's slot
// is written with zeros (grid-stride).  Plain vector stores.
__global__ __launch_bounds__(256) void k_jpegdec_zero(JpegDecArgs a)
{
    const Frame &f = reinterpret_cast<const Frame *>(a.blob + a.frames_off)[blockIdx.y];
    if (f.raw) return;
    const int *status = reinterpret_cast<const int *>(a.blob + a.status_off);
    int bad = status[blockIdx.y];
    for (int s = (int)threadIdx.x; s < f.n_seg; s += 256) bad |= status[a.n_frames + f.first_seg + s];
    if (!__syncthreads_or(bad)) return;
    const size_t bytes = (size_t)f.width * f.height * 3;
    uint8_t *out = a.rgb + f.rgb_off;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < bytes; i += (size_t)gridDim.x * 256) out[i] = 0;
}

}  // namespace y2jpg
