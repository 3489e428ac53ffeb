// kernels_draw.hpp -- the annotated frame on the GPU: source pixels in their camera format -> packed RGB24 with the boxes and tags of
// the reference's yolo2_draw_detections_rgb24 (linux_app/src/yolo2_draw.c:276-369) painted in, one read and one write per pixel.
//
// The reference paints record after record into the frame, later records over earlier ones, per record the border, the tag's
// rectangle, the glyphs.  Here every output pixel asks the frame's draw list (draw_list.hpp: one DrawItem per drawn record, made on
// the host) from its LAST item back to its first and takes the first item that covers it - within an item the tag (glyph bit: text
// colour, else the tag's colour) before the two border rings.  That is the painter's result without a write race: a pixel is
// stored once.  Glyph pixels need no test of their own outside the tag: every glyph pixel inside the image lies inside the clamped
// tag rectangle (the text sits 2 pixels inside the unclamped one, and the clamp only cuts at the image's edges).
//
// Work split: a frame's pixels are one flat run (packed RGB24 has no row padding); a workgroup takes a strip of kAnnoStripPx
// consecutive pixels, a lane kAnnoGroups runs of 4 pixels = 12 bytes = 3 dwords of it.  A run is loaded and stored as dwords where
// the frame's base is 4-byte aligned and the run is whole, and byte by byte otherwise (a frame's last, short run; a caller's odd
// address).  A workgroup stages in LDS the items whose extent (box united with tag) meets the rows of its strip, kAnnoPiece items
// of the list at a time, in list order from the back.  A frame without items is a pure convert / copy.
//
// Launched from yolo2_draw.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "draw_list.hpp"
#include "letterbox.hpp"

namespace y2 {

using y2d::DrawItem;

// The table that leads a chunk's staging buffer (LetterboxItem leads the letterbox chunk the same way): header, one AnnoFrame per
// frame, the draw items of all frames.
struct AnnoHeader {
    uint64_t font[y2d::kDrawGlyphs];   // y2d::kDrawFont
    unsigned long long items_off;      // where the DrawItem array starts, in bytes from the table
};
struct AnnoFrame {
    unsigned long long src_off, out_off;   // the frame's source bytes / its RGB24 output, in bytes from the two base addresses
    int w, h, ch;                          // ch: source bytes per pixel - 1 grey, 3 RGB24, 2 packed YUYV 4:2:2 (w even, 4-byte aligned);
                                           // kLbChNv12 / kLbChI420: planar YUV 4:2:0 (w and h even, any address); kLbChBgr24: packed
                                           // B G R (any address); kLbChRgba32 / kLbChBgra32: R G B X / B G R X dwords (4-byte aligned)
    int item0, n_items;                    // its items in the array, in record order
    int strips;                            // workgroups that have work on it: ceil(w * h / kAnnoStripPx)
};

constexpr int kAnnoThreads = 256, kAnnoGroups = 4, kAnnoStripPx = kAnnoThreads * kAnnoGroups * 4, kAnnoPiece = 128;
constexpr int kAnnoItemDwords = (int)(sizeof(DrawItem) / 4);
static_assert(sizeof(DrawItem) % 4 == 0 && kAnnoPiece <= kAnnoThreads, "items are copied dword by dword, one lane tests one item");

// One pixel of a loaded YUYV pair (bytes Y0 U Y1 V) -> R | G << 8 | B << 16: the conversion of the YUYV entries (letterbox.hpp, LbYuyv
// - its arithmetic on a dword that is loaded once per pair; tests/test_gpu_draw.py holds the two together)
__device__ inline uint32_t anno_yuyv_px(uint32_t pair, int odd)
{
    const int c = 298 * ((int)((pair >> (odd * 16)) & 255u) - 16) + 128, d = (int)((pair >> 8) & 255u) - 128, e = (int)(pair >> 24) - 128;
    const int r = min(max((c + 409 * e) >> 8, 0), 255), g = min(max((c - 100 * d - 208 * e) >> 8, 0), 255), b = min(max((c + 516 * d) >> 8, 0), 255);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

// Pixel (x, y) of a planar 4:2:0 frame (letterbox.hpp, LbYuv420: Y plane, then NV12's interleaved U V plane or I420's U and V planes;
// byte loads, the frame may start anywhere) as the YUYV pair it stands for
__device__ inline uint32_t anno_yuv420_px(const uint8_t *__restrict__ src, int w, int h, bool semi, int x, int y)
{
    const uint8_t *c = src + (size_t)w * h;
    const size_t at = semi ? (size_t)(y >> 1) * w + (x & ~1) : (size_t)(y >> 1) * (w >> 1) + (x >> 1);
    const uint32_t u = c[at], v = semi ? c[at + 1] : c[at + (size_t)(w >> 1) * (h >> 1)];
    return anno_yuyv_px((uint32_t)src[(size_t)y * w + x] | (u << 8) | (v << 24), 0);
}

// c with bytes 0 and 2 exchanged and byte 3 cleared: B G R [X] <-> R | G << 8 | B << 16, one v_perm_b32
__device__ inline uint32_t anno_swap_rb(uint32_t c) { return __byte_perm(c, 0u, 0x4012u); }

// source pixel p of a frame -> R | G << 8 | B << 16
__device__ inline uint32_t anno_load_px(const uint8_t *__restrict__ src, int ch, int p)
{
    if (ch == kLbChBgr24) return (uint32_t)src[(size_t)p * 3 + 2] | ((uint32_t)src[(size_t)p * 3 + 1] << 8) | ((uint32_t)src[(size_t)p * 3] << 16);
    if (ch == kLbChRgba32) return reinterpret_cast<const uint32_t *>(src)[p] & 0xffffffu;   // (the fourth byte is dropped here)
    if (ch == kLbChBgra32) return anno_swap_rb(reinterpret_cast<const uint32_t *>(src)[p]);
    if (ch == 3) return (uint32_t)src[(size_t)p * 3] | ((uint32_t)src[(size_t)p * 3 + 1] << 8) | ((uint32_t)src[(size_t)p * 3 + 2] << 16);
    if (ch == 1) return (uint32_t)src[p] * 0x010101u;
    return anno_yuyv_px(reinterpret_cast<const uint32_t *>(src)[p >> 1], p & 1);   // (the frame as one row of pairs)
}

// does `it` paint pixel (x, y)?  c: the colour it leaves there
__device__ inline bool anno_hit(const DrawItem &it, const uint64_t *font, int x, int y, uint32_t &c)
{
    if (x < it.ext[0] || x > it.ext[2] || y < it.ext[1] || y > it.ext[3]) return false;
    if (x >= it.tag[0] && x <= it.tag[2] && y >= it.tag[1] && y <= it.tag[3]) {
        c = it.box_rgb;
        const int dx = x - it.gx, dy = y - it.gy;
        if (dx >= 0 && dy >= 0 && dy < y2d::kDrawGlyphH && dx < it.nchar * y2d::kDrawCell) {
            const int k = dx / y2d::kDrawCell, cx = (dx - k * y2d::kDrawCell) / y2d::kDrawScale;
            if (cx < 5 && ((font[it.text[k]] >> (5 * (dy / y2d::kDrawScale) + cx)) & 1)) c = it.text_rgb;
        }
        return true;
    }
#pragma unroll
    for (int t = 0; t < y2d::kDrawThick; ++t) {
        const int *r = it.ring[t];
        if (((y == r[1] || y == r[3]) && x >= r[0] && x <= r[2]) || ((x == r[0] || x == r[2]) && y >= r[1] && y <= r[3])) {
            c = it.box_rgb;
            return true;
        }
    }
    return false;
}

// The draw list made on the device: a chunk's compact records (k_compact_dets, YOLO2_DETS_BEST_CLASS form: [frames][cap] with the
// per-frame counts) -> the table k_annotate_batch reads.  One workgroup per frame.  `geom` is the table as the host can know it
// before the records exist - AnnoHeader (font, items_off) and AnnoFrame[frames] with everything but item0 / n_items - and `table` the
// complete one: header and frames copied, frame f's items at item0 = f * cap in RECORD order (the order decides which item paints
// last), made by y2d::draw_item_from_record, the arithmetic the host twin (y2h_draw_item) runs.  The drawn records are compacted in
// order with an exclusive scan over pieces of 1024 records (4 consecutive records per lane, as k_compact_dets scans its rows).
// info [2 * frames]: n_items, and the records that would be drawn but whose prob the formatter does not print (not drawn, counted).
// labels: n_labels entries of y2d::draw_label_entry, or NULL.  Plain vector stores only; frames are independent.
constexpr int kItemsThreads = 256, kItemsPiece = kItemsThreads * 4;
__global__ __launch_bounds__(kItemsThreads) void k_draw_items(const y2d::DrawDet *__restrict__ dets, const int *__restrict__ counts, int cap,
                                                              float thresh, const uint8_t *__restrict__ labels, int n_labels,
                                                              const uint8_t *__restrict__ geom, uint8_t *__restrict__ table,
                                                              int *__restrict__ info)
{
    __shared__ int s_wave[kItemsThreads / 64], s_bad[kItemsThreads / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AnnoHeader *gh = reinterpret_cast<const AnnoHeader *>(geom);
    const AnnoFrame gf = reinterpret_cast<const AnnoFrame *>(geom + sizeof(AnnoHeader))[f];
    const unsigned long long items_off = gh->items_off;
    if (f == 0) {
        AnnoHeader *th = reinterpret_cast<AnnoHeader *>(table);
        if (tid < y2d::kDrawGlyphs) th->font[tid] = gh->font[tid];
        if (tid == 0) th->items_off = items_off;
    }
    const int n = min(max(counts[f], 0), cap);
    const y2d::DrawDet *rec = dets + (size_t)f * cap;
    DrawItem *items = reinterpret_cast<DrawItem *>(table + items_off) + (size_t)f * cap;
    int base = 0, bad = 0;
    for (int p0 = 0; p0 < n; p0 += kItemsPiece) {   // (uniform: n is the frame's)
        int v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = p0 + tid * 4 + k;
            v[k] = 0;
            if (i < n) {
                const y2d::DrawDet d = rec[i];
                if (y2d::draw_is_drawn(d, thresh)) {
                    if (y2d::draw_prob_printable(d.prob)) v[k] = 1;
                    else ++bad;
                }
            }
            s += v[k];
        }
        int incl = s;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        __syncthreads();   // the piece before has read s_wave
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kItemsThreads / 64; ++w) { if (w < wave) before += s_wave[w]; total += s_wave[w]; }
        int at = base + before + incl - s;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (v[k]) {   // at < n <= cap: inside the frame's cap items
                bool unprintable;
                (void)y2d::draw_item_from_record(rec[p0 + tid * 4 + k], gf.w, gf.h, thresh, labels, n_labels, &items[at], &unprintable);
                ++at;
            }
        base += total;
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    __syncthreads();
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    if (tid == 0) {
        AnnoFrame out = gf;
        out.item0 = f * cap;
        out.n_items = base;
        reinterpret_cast<AnnoFrame *>(table + sizeof(AnnoHeader))[f] = out;
        info[2 * f] = base;
        int b = 0;
        for (int w = 0; w < kItemsThreads / 64; ++w) b += s_bad[w];
        info[2 * f + 1] = b;
    }
}

// The painter's body.  BGR: the output frame is packed B G R instead of R G B - one byte permute per pixel before the store.
template <bool BGR>
__device__ __forceinline__ void annotate_batch_tiles(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                     uint8_t *__restrict__ out_base)
{
    __shared__ uint64_t s_font[y2d::kDrawGlyphs];
    __shared__ DrawItem s_items[kAnnoPiece];
    __shared__ int s_sel[kAnnoPiece];
    __shared__ int s_wave[kAnnoThreads / 64];

    const AnnoHeader *hd = reinterpret_cast<const AnnoHeader *>(table);
    const AnnoFrame fr = reinterpret_cast<const AnnoFrame *>(table + sizeof(AnnoHeader))[blockIdx.y];
    if ((int)blockIdx.x >= fr.strips) return;   // (the whole workgroup)
    const DrawItem *items = reinterpret_cast<const DrawItem *>(table + hd->items_off) + fr.item0;
    const int tid = threadIdx.x;
    if (tid < y2d::kDrawGlyphs) s_font[tid] = hd->font[tid];

    const int npx = fr.w * fr.h;
    const int p_lo = (int)blockIdx.x * kAnnoStripPx, p_hi = min(npx, p_lo + kAnnoStripPx);
    const int ya = p_lo / fr.w, yb = (p_hi - 1) / fr.w;   // the rows this strip touches
    const uint8_t *src = src_base + fr.src_off;
    uint8_t *out = out_base + fr.out_off;
    const bool src_al = ((uintptr_t)src & 3) == 0, out_al = ((uintptr_t)out & 3) == 0;

    // ---- this lane's pixels: run j starts at pixel p_lo + (j * 256 + tid) * 4
    uint32_t col[kAnnoGroups * 4];
    int px[kAnnoGroups * 4], py[kAnnoGroups * 4];
    unsigned todo = 0;   // bit k: pixel k exists and no item has painted it yet
#pragma unroll
    for (int j = 0; j < kAnnoGroups; ++j) {
        const int p = p_lo + (j * kAnnoThreads + tid) * 4;
        if (p >= p_hi) continue;
        const bool whole = p + 4 <= p_hi;
        if (whole && src_al && fr.ch == 3) {
            const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 3);
            const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
            col[4 * j] = d0 & 0xffffffu;
            col[4 * j + 1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
            col[4 * j + 2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
            col[4 * j + 3] = d2 >> 8;
        } else if (whole && src_al && fr.ch == kLbChBgr24) {   // RGB24's three dwords, every pixel's bytes 0 and 2 exchanged
            const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 3);
            const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
            col[4 * j] = anno_swap_rb(d0);
            col[4 * j + 1] = anno_swap_rb((d0 >> 24) | (d1 << 8));
            col[4 * j + 2] = anno_swap_rb((d1 >> 16) | (d2 << 16));
            col[4 * j + 3] = anno_swap_rb(d2 >> 8);
        } else if (whole && (fr.ch == kLbChRgba32 || fr.ch == kLbChBgra32)) {   // one dword per pixel (4-byte aligned, as YUYV)
            const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) col[4 * j + i] = fr.ch == kLbChBgra32 ? anno_swap_rb(s[i]) : (s[i] & 0xffffffu);
        } else if (whole && fr.ch == 2) {   // (a YUYV frame starts on a 4-byte boundary: the entries refuse any other)
            const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 2);
            const uint32_t d0 = s[0], d1 = s[1];
            col[4 * j] = anno_yuyv_px(d0, 0);
            col[4 * j + 1] = anno_yuyv_px(d0, 1);
            col[4 * j + 2] = anno_yuyv_px(d1, 0);
            col[4 * j + 3] = anno_yuyv_px(d1, 1);
        } else if (fr.ch == kLbChNv12 || fr.ch == kLbChI420) {   // a run may cross a row's end: (x, y) per pixel
            const int y0 = p / fr.w;
            int x = p - y0 * fr.w, y = y0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                col[4 * j + i] = p + i < p_hi ? anno_yuv420_px(src, fr.w, fr.h, fr.ch == kLbChNv12, x, y) : 0u;
                if (++x == fr.w) { x = 0; ++y; }
            }
        } else if (whole && src_al && fr.ch == 1) {
            const uint32_t d = *reinterpret_cast<const uint32_t *>(src + p);
#pragma unroll
            for (int i = 0; i < 4; ++i) col[4 * j + i] = ((d >> (8 * i)) & 255u) * 0x010101u;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) col[4 * j + i] = p + i < p_hi ? anno_load_px(src, fr.ch, p + i) : 0u;
        }
        const int y0 = p / fr.w;
        int x = p - y0 * fr.w, y = y0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            px[4 * j + i] = x;
            py[4 * j + i] = y;
            if (p + i < p_hi) todo |= 1u << (4 * j + i);
            if (++x == fr.w) { x = 0; ++y; }
        }
    }

    // ---- the draw list from the back, kAnnoPiece items at a time
    for (int hi = fr.n_items; hi > 0; hi -= kAnnoPiece) {
        const int cnt = min(kAnnoPiece, hi);
        __syncthreads();   // the piece before this one has been read by everybody (first time round: s_font is written)
        // lane t looks at item hi - 1 - t; the items that meet the strip keep that order in s_sel
        bool meets = false;
        if (tid < cnt) {
            const DrawItem &g = items[hi - 1 - tid];
            meets = g.ext[1] <= yb && g.ext[3] >= ya;
        }
        const unsigned long long m = __ballot(meets);
        const int wave = tid >> 6, lane = tid & 63;
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, nsel = 0;
#pragma unroll
        for (int v = 0; v < kAnnoThreads / 64; ++v) {
            if (v < wave) before += s_wave[v];
            nsel += s_wave[v];
        }
        if (meets) s_sel[before + __popcll(m & ((1ull << lane) - 1ull))] = hi - 1 - tid;
        __syncthreads();
        for (int e = tid; e < nsel * kAnnoItemDwords; e += kAnnoThreads) {
            const int s = e / kAnnoItemDwords, d = e - s * kAnnoItemDwords;
            reinterpret_cast<uint32_t *>(s_items)[e] = reinterpret_cast<const uint32_t *>(items + s_sel[s])[d];
        }
        __syncthreads();
        for (int s = 0; s < nsel && todo; ++s) {
            const DrawItem &it = s_items[s];
#pragma unroll
            for (int k = 0; k < kAnnoGroups * 4; ++k) {
                uint32_t c;
                if (((todo >> k) & 1u) && anno_hit(it, s_font, px[k], py[k], c)) {
                    col[k] = c;
                    todo &= ~(1u << k);
                }
            }
        }
    }

    // ---- packed RGB24 out
    if constexpr (BGR) {
#pragma unroll
        for (int k = 0; k < kAnnoGroups * 4; ++k) col[k] = anno_swap_rb(col[k]);
    }
#pragma unroll
    for (int j = 0; j < kAnnoGroups; ++j) {
        const int p = p_lo + (j * kAnnoThreads + tid) * 4;
        if (p >= p_hi) continue;
        if (p + 4 <= p_hi && out_al) {
            uint32_t *o = reinterpret_cast<uint32_t *>(out + (size_t)p * 3);
            const uint32_t c0 = col[4 * j] & 0xffffffu, c1 = col[4 * j + 1] & 0xffffffu, c2 = col[4 * j + 2] & 0xffffffu, c3 = col[4 * j + 3] & 0xffffffu;
            o[0] = c0 | (c1 << 24);
            o[1] = (c1 >> 8) | (c2 << 16);
            o[2] = (c2 >> 16) | (c3 << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (p + i >= p_hi) break;
                uint8_t *o = out + (size_t)(p + i) * 3;
                o[0] = (uint8_t)col[4 * j + i];
                o[1] = (uint8_t)(col[4 * j + i] >> 8);
                o[2] = (uint8_t)(col[4 * j + i] >> 16);
            }
        }
    }
}

// grid (max strips of the chunk's frames, frames); table: AnnoHeader, AnnoFrame[frames], DrawItem[]
__global__ __launch_bounds__(kAnnoThreads) void k_annotate_batch(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                                 uint8_t *__restrict__ out_base)
{
    annotate_batch_tiles<false>(table, src_base, out_base);
}

// the same into packed BGR24 frames, what cv2.imshow / cv2.VideoWriter take (the loop's YOLO2_LOOP_OUT_BGR24)
__global__ __launch_bounds__(kAnnoThreads) void k_annotate_batch_bgr(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                                     uint8_t *__restrict__ out_base)
{
    annotate_batch_tiles<true>(table, src_base, out_base);
}

// ---- The painter into planar YUV 4:2:0 frames (the loop's YOLO2_LOOP_OUT_NV12 / _I420, include/yolo2_hip.h): the RGB24 frame the
// painter above leaves, converted where it would be stored -
//   per pixel      Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
//   per 2x2 block  U = ((-38 Rs - 74 Gs + 112 Bs + 512) >> 10) + 128,  V = ((112 Rs - 94 Gs - 18 Bs + 512) >> 10) + 128
// (Rs, Gs, Bs: the sums over the block; arithmetic shifts; Y in 16..235 and U, V in 16..240 for every colour, so nothing is clamped).
// A chroma byte needs a whole 2x2 block, so the flat mapping above does not serve: here a frame is a grid of PATCHES, 4 pixels wide
// and 2 rows high (two blocks; the last patch of a row is 2 wide where w % 4 == 2), numbered row by row, ceil(w / 4) * (h / 2) of them.
// A workgroup takes kAnnoYuvStrip consecutive patches, a lane kAnnoYuvPatches of them (patch j * 256 + tid of the strip) = 16 pixels,
// the flat painter's count.  Per patch: two runs of 4 source pixels in, two dwords of Y, and one dword U V U V (NV12) or two bytes
// each of U and V (I420) out.  Every wide store is taken only where its own byte offset allows it - a Y row starts on a dword only
// where y * w does (w % 4 == 2: every other row), an I420 chroma row (w / 2 bytes) and the V plane ((w / 2) * (h / 2) bytes behind U)
// may start on any byte - and falls back to byte stores; each output byte is still written once.  The source fetch, the staging of
// the items that meet the workgroup's rows and the walk from the back of the list are the flat painter's.  AnnoFrame::strips
// describes the flat mapping and is not read here: the workgroup count comes from anno_yuv_groups, on both sides of the launch.
constexpr int kAnnoYuvPatches = 2, kAnnoYuvStrip = kAnnoThreads * kAnnoYuvPatches;
static_assert(kAnnoYuvPatches * 8 == kAnnoGroups * 4, "a lane holds as many pixels as in the flat painter");

// workgroups that have work on a w x h frame (w, h even)
__host__ __device__ inline int anno_yuv_groups(int w, int h)
{
    return (int)((((long long)((w + 3) >> 2)) * (h >> 1) + kAnnoYuvStrip - 1) / kAnnoYuvStrip);
}

// pixels x .. x + n - 1 (n = 2 or 4, x % 4 == 0) of row y -> c[0 .. n - 1] as R | G << 8 | B << 16, the rest of c[0..3] zero
__device__ __forceinline__ void anno_load_row4(const uint8_t *__restrict__ src, const AnnoFrame &fr, bool src_al, int x, int y, int n, uint32_t *c)
{
    const int p = y * fr.w + x;
    const bool whole = n == 4, al = whole && src_al && (p & 3) == 0;   // al: the run's 12 (grey: 4) bytes start on a dword
    if (al && fr.ch == 3) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 3);
        const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
        c[0] = d0 & 0xffffffu;
        c[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
        c[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
        c[3] = d2 >> 8;
    } else if (al && fr.ch == kLbChBgr24) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 3);
        const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
        c[0] = anno_swap_rb(d0);
        c[1] = anno_swap_rb((d0 >> 24) | (d1 << 8));
        c[2] = anno_swap_rb((d1 >> 16) | (d2 << 16));
        c[3] = anno_swap_rb(d2 >> 8);
    } else if (whole && (fr.ch == kLbChRgba32 || fr.ch == kLbChBgra32)) {   // (4-byte aligned frames, one dword per pixel)
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = fr.ch == kLbChBgra32 ? anno_swap_rb(s[i]) : (s[i] & 0xffffffu);
    } else if (whole && fr.ch == 2) {   // (a YUYV frame is 4-byte aligned and w is even, so p is even: whole pairs)
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + (size_t)p * 2);
        const uint32_t d0 = s[0], d1 = s[1];
        c[0] = anno_yuyv_px(d0, 0);
        c[1] = anno_yuyv_px(d0, 1);
        c[2] = anno_yuyv_px(d1, 0);
        c[3] = anno_yuyv_px(d1, 1);
    } else if (fr.ch == kLbChNv12 || fr.ch == kLbChI420) {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = i < n ? anno_yuv420_px(src, fr.w, fr.h, fr.ch == kLbChNv12, x + i, y) : 0u;
    } else if (al && fr.ch == 1) {
        const uint32_t d = *reinterpret_cast<const uint32_t *>(src + p);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = ((d >> (8 * i)) & 255u) * 0x010101u;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = i < n ? anno_load_px(src, fr.ch, p + i) : 0u;
    }
}

__device__ __forceinline__ uint32_t anno_luma(uint32_t c)
{
    return (uint32_t)(((66 * (int)(c & 255u) + 129 * (int)((c >> 8) & 255u) + 25 * (int)((c >> 16) & 255u) + 128) >> 8) + 16);
}

// U | V << 8 of the 2x2 block a b / c d
__device__ __forceinline__ uint32_t anno_chroma(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const int rs = (int)((a & 255u) + (b & 255u) + (c & 255u) + (d & 255u));
    const int gs = (int)(((a >> 8) & 255u) + ((b >> 8) & 255u) + ((c >> 8) & 255u) + ((d >> 8) & 255u));
    const int bs = (int)(((a >> 16) & 255u) + ((b >> 16) & 255u) + ((c >> 16) & 255u) + ((d >> 16) & 255u));
    const int u = ((-38 * rs - 74 * gs + 112 * bs + 512) >> 10) + 128, v = ((112 * rs - 94 * gs - 18 * bs + 512) >> 10) + 128;
    return (uint32_t)u | ((uint32_t)v << 8);
}

// n (2 or 4) bytes of dword v at out + off: one dword store where n == 4 and the address allows it, bytes otherwise
__device__ __forceinline__ void anno_store_bytes(uint8_t *__restrict__ out, bool out_al, size_t off, uint32_t v, int n)
{
    if (n == 4 && out_al && (off & 3) == 0) {
        *reinterpret_cast<uint32_t *>(out + off) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) out[off + i] = (uint8_t)(v >> (8 * i));
    }
}

// SEMI: NV12's interleaved U V plane; otherwise I420's U and V planes
template <bool SEMI>
__device__ __forceinline__ void annotate_batch_yuv420(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                      uint8_t *__restrict__ out_base)
{
    __shared__ uint64_t s_font[y2d::kDrawGlyphs];
    __shared__ DrawItem s_items[kAnnoPiece];
    __shared__ int s_sel[kAnnoPiece];
    __shared__ int s_wave[kAnnoThreads / 64];

    const AnnoHeader *hd = reinterpret_cast<const AnnoHeader *>(table);
    const AnnoFrame fr = reinterpret_cast<const AnnoFrame *>(table + sizeof(AnnoHeader))[blockIdx.y];
    if ((int)blockIdx.x >= anno_yuv_groups(fr.w, fr.h)) return;   // (the whole workgroup)
    const DrawItem *items = reinterpret_cast<const DrawItem *>(table + hd->items_off) + fr.item0;
    const int tid = threadIdx.x;
    if (tid < y2d::kDrawGlyphs) s_font[tid] = hd->font[tid];

    const int pw = (fr.w + 3) >> 2, npatch = pw * (fr.h >> 1);   // patches per patch row, patches of the frame
    const int q_lo = (int)blockIdx.x * kAnnoYuvStrip, q_hi = min(npatch, q_lo + kAnnoYuvStrip);
    const int ya = 2 * (q_lo / pw), yb = 2 * ((q_hi - 1) / pw) + 1;   // the rows this strip touches
    const uint8_t *src = src_base + fr.src_off;
    uint8_t *out = out_base + fr.out_off;
    const bool src_al = ((uintptr_t)src & 3) == 0, out_al = ((uintptr_t)out & 3) == 0;

    // ---- this lane's pixels: patch j is patch q_lo + j * 256 + tid, its pixel (x0 + i, y0 + r) is col[8 * j + 4 * r + i]
    uint32_t col[kAnnoYuvPatches * 8];
    int x0[kAnnoYuvPatches], y0[kAnnoYuvPatches], pn[kAnnoYuvPatches];   // pn: the patch's width, 0 where the lane has none
    unsigned todo = 0;   // bit k: pixel k exists and no item has painted it yet
#pragma unroll
    for (int j = 0; j < kAnnoYuvPatches; ++j) {
        const int q = q_lo + j * kAnnoThreads + tid;
        x0[j] = y0[j] = pn[j] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) col[8 * j + k] = 0u;
        if (q >= q_hi) continue;
        const int pr = q / pw;
        x0[j] = (q - pr * pw) * 4;
        y0[j] = pr * 2;
        pn[j] = min(4, fr.w - x0[j]);
        anno_load_row4(src, fr, src_al, x0[j], y0[j], pn[j], &col[8 * j]);
        anno_load_row4(src, fr, src_al, x0[j], y0[j] + 1, pn[j], &col[8 * j + 4]);
        todo |= (pn[j] == 4 ? 0xffu : 0x33u) << (8 * j);
    }

    // ---- the draw list from the back, kAnnoPiece items at a time (the flat painter's staging)
    for (int hi = fr.n_items; hi > 0; hi -= kAnnoPiece) {
        const int cnt = min(kAnnoPiece, hi);
        __syncthreads();   // the piece before this one has been read by everybody (first time round: s_font is written)
        bool meets = false;
        if (tid < cnt) {
            const DrawItem &g = items[hi - 1 - tid];
            meets = g.ext[1] <= yb && g.ext[3] >= ya;
        }
        const unsigned long long m = __ballot(meets);
        const int wave = tid >> 6, lane = tid & 63;
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, nsel = 0;
#pragma unroll
        for (int v = 0; v < kAnnoThreads / 64; ++v) {
            if (v < wave) before += s_wave[v];
            nsel += s_wave[v];
        }
        if (meets) s_sel[before + __popcll(m & ((1ull << lane) - 1ull))] = hi - 1 - tid;
        __syncthreads();
        for (int e = tid; e < nsel * kAnnoItemDwords; e += kAnnoThreads) {
            const int s = e / kAnnoItemDwords, d = e - s * kAnnoItemDwords;
            reinterpret_cast<uint32_t *>(s_items)[e] = reinterpret_cast<const uint32_t *>(items + s_sel[s])[d];
        }
        __syncthreads();
        for (int s = 0; s < nsel && todo; ++s) {
            const DrawItem &it = s_items[s];
#pragma unroll
            for (int k = 0; k < kAnnoYuvPatches * 8; ++k) {
                uint32_t c;
                if (((todo >> k) & 1u) && anno_hit(it, s_font, x0[k >> 3] + (k & 3), y0[k >> 3] + ((k >> 2) & 1), c)) {
                    col[k] = c;
                    todo &= ~(1u << k);
                }
            }
        }
    }

    // ---- planar 4:2:0 out
    const size_t ysize = (size_t)fr.w * fr.h;
#pragma unroll
    for (int j = 0; j < kAnnoYuvPatches; ++j) {
        const int n = pn[j];
        if (!n) continue;
        const uint32_t *c = &col[8 * j];
#pragma unroll
        for (int r = 0; r < 2; ++r)
            anno_store_bytes(out, out_al, (size_t)(y0[j] + r) * fr.w + x0[j],
                             anno_luma(c[4 * r]) | (anno_luma(c[4 * r + 1]) << 8) | (anno_luma(c[4 * r + 2]) << 16) | (anno_luma(c[4 * r + 3]) << 24), n);
        const uint32_t uv0 = anno_chroma(c[0], c[1], c[4], c[5]), uv1 = anno_chroma(c[2], c[3], c[6], c[7]);   // (uv1 of a 2-wide patch is not stored)
        if constexpr (SEMI) {
            anno_store_bytes(out, out_al, ysize + (size_t)(y0[j] >> 1) * fr.w + x0[j], uv0 | (uv1 << 16), n);
        } else {
            const size_t cw = (size_t)(fr.w >> 1), at = ysize + (size_t)(y0[j] >> 1) * cw + (x0[j] >> 1), vplane = cw * (fr.h >> 1);
            const uint32_t uu = (uv0 & 255u) | ((uv1 & 255u) << 8), vv = (uv0 >> 8) | (uv1 & 0xff00u);
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {   // U, then V
                const size_t off = at + (pl ? vplane : 0);
                const uint32_t b2 = pl ? vv : uu;
                if (n == 4 && out_al && (off & 1) == 0) {
                    *reinterpret_cast<uint16_t *>(out + off) = (uint16_t)b2;
                } else {
                    out[off] = (uint8_t)b2;
                    if (n == 4) out[off + 1] = (uint8_t)(b2 >> 8);
                }
            }
        }
    }
}

// grid (max anno_yuv_groups of the chunk's frames, frames); the table of k_annotate_batch.  Frames: Y [h][w], then U V rows [h/2][w]
__global__ __launch_bounds__(kAnnoThreads) void k_annotate_batch_nv12(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                                      uint8_t *__restrict__ out_base)
{
    annotate_batch_yuv420<true>(table, src_base, out_base);
}

// ... Y [h][w], then U [h/2][w/2], then V [h/2][w/2]
__global__ __launch_bounds__(kAnnoThreads) void k_annotate_batch_i420(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                                      uint8_t *__restrict__ out_base)
{
    annotate_batch_yuv420<false>(table, src_base, out_base);
}

}  // namespace y2
