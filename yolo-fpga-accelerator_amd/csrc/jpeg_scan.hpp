// jpeg_scan.hpp -- the stages of the baseline JPEG decoder as functions that run on the device and on the host (the precedent is
// draw_list.hpp): the bit reader, Huffman symbol and RECEIVE + EXTEND, one sequential block, one restart interval ("segment"), the inverse
// DCT, and the up-sampling + colour formulas as a function of the output pixel.  They restate host/y2_codec.cpp (Bits, block_sequential,
// interval_done, idct_block, row_*, ycc_to_rgb), which is the expected side of every test and stays as it is.  Users: the kernels
// (kernels_jpegdec.hpp), the host doorway yolo2_hip_decode_jpeg_ref (jpeg_parse.hpp: y2jpg::decode_ref) and tools/fuzz_jpegdec.cpp.
// Behind decode_segment: one segment decoded by many lanes (option jpegdec_split) - a reader whose positions are canonical (SBits), one
// subsequence from a given state (split_run) and the acceptance rule; users k_jpegdec_split, yolo2_hip_decode_jpeg_split_ref
// (jpeg_parse.hpp: split_segment_host) and tools/fuzz_jpegdec_split.cpp.
// Plain C++ for a host compiler, __host__ __device__ under hipcc.  Integer arithmetic wraps as the host's does (-fwrapv on both sides).
//
// What differs from the host's walk, and why the bytes are the same:
//   * a frame is decoded segment by segment - one restart interval each, found by a byte scan for RSTn (jpeg_parse.hpp) - and every
//     segment starts from a reset reader and zero DC predictions, which is what Jpeg::restart() leaves.  The host's result depends on
//     nothing else carried across intervals AS LONG AS every interval ends at its marker; where one does not (interval_done gives up),
//     where the number of markers does not fit the geometry, or where the last interval does not end at the marker that closes the
//     scan, the frame is flagged (kRestartOutOfStep) instead of decoded;
//   * the inverse DCT has no all-AC-zero column shortcut: (d * 4096 + 512) >> 10 == 4 d for every int d, and with s[1..7] == 0 idct_1d
//     returns x[k] = 4096 s[0], t[k] = 0 - the general path gives the shortcut's value;
//   * jpeg_to_rgb's row walk (line0 / line1 / ystep) written out per output row: with vs == 2 row 2k reads near = plane row k and far =
//     max(k - 1, 0), row 2k + 1 near = k and far = min(k + 1, comp.y - 1); the horizontal filters replicate at w_lores.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define Y2J_HD __host__ __device__
#else
#define Y2J_HD
#endif

namespace y2jpg {

enum Status { kOk = 0, kBadCode = 1, kCoefOverrun = 2, kRestartOutOfStep = 3 };

// (namespace scope: a table inside the function would be built in each lane's scratch memory on the device)
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
Y2J_HD inline int zigzag(int i) { return kZigzag[i]; }

// Canonical Huffman table as the decoder reads it: look[9-bit prefix] = length << 8 | symbol for codes of <= 9 bits (0: none), the
// T.81 F.2.2.3 arrays for the longer ones.  1488 bytes, a multiple of 16 (the kernel copies table sets to LDS in 16-byte pieces).
struct Huff {
    uint16_t look[512];
    int32_t maxcode[17], mincode[17], valptr[17];
    uint8_t vals[256];
    uint32_t defined;
};
// What one frame's scan reads: its components' tables in FRAME order (a table two components name is stored twice), and their
// quantisation tables in natural order.  Identical sets inside a chunk are stored once.
struct Tables {
    Huff dc[3], ac[3];
    uint16_t q[3][64];
};
static_assert(sizeof(Huff) == 1488 && sizeof(Tables) % 16 == 0, "table sets are copied in 16-byte pieces");

struct Comp {
    int h, v;          // sampling factors (a single component: 1, 1 - its scan is its own blocks in raster order)
    int x, y;          // effective samples
    int w2, h2;        // plane (whole MCUs); the coefficient buffer holds (h2 / 8) x (w2 / 8) blocks of 64 in the same order
    uint32_t off;      // of the plane within the frame's planes, in samples; the same number is its offset in coefficients
};
struct Frame {
    int width, height, ncomp, hmax, vmax, mcu_x, mcu_y, restart_interval;
    int order[3];      // scan position -> component
    Comp comp[3];
    int tables;        // table set
    int raw;           // 1: the caller's RGB24 bytes are the frame (no stream): every stage skips it
    int first_seg, n_seg;
    int blocks;        // all components'
    uint32_t samples;  // all planes'
    unsigned long long coef_off, plane_off, rgb_off;   // of this frame within the chunk's buffers (coefficients, samples, bytes)
};
// One restart interval (or the whole scan): bytes [begin, end) of the chunk's stream buffer - the marker that ends it included - and the
// MCUs it holds.  `last`: the scan's last interval, which must end at the marker that closes the scan.
struct Segment {
    uint32_t begin, end;
    int frame, first_mcu, n_mcu, last;
};

// MSB-first bit reader over one segment.  0xFF00 is a data byte 0xFF, 0xFF followed by anything else is a marker: reading stops there
// and zero bits follow (Bits of y2_codec.cpp).  Nothing outside [p, end) is used; past `end` zero bits follow too.  On the device the
// bytes come from the aligned 16-byte piece that holds them, loaded once (base is 16-byte aligned and the buffer is padded to a
// multiple of 16, so the piece is inside the allocation; bytes of it outside [begin, end) are never looked at).
struct Bits {
    const uint8_t *base;
    uint32_t p, end;
    uint32_t acc;
    int n, marker;
    bool dry;
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 piece;
    uint32_t piece_at;
#endif
    Y2J_HD void open(const uint8_t *b, uint32_t begin, uint32_t e)
    {
        base = b; p = begin; end = e; acc = 0; n = 0; marker = -1; dry = false;
#if defined(__HIP_DEVICE_COMPILE__)
        piece_at = 0xffffffffu;
        piece = make_uint4(0, 0, 0, 0);
#endif
    }
#if defined(__HIP_DEVICE_COMPILE__)
    __device__ void shift8()
    {
        piece.x = (piece.x >> 8) | (piece.y << 24); piece.y = (piece.y >> 8) | (piece.z << 24);
        piece.z = (piece.z >> 8) | (piece.w << 24); piece.w >>= 8;
    }
#endif
    Y2J_HD uint32_t next()   // the byte at p (p < end), p advanced
    {
#if defined(__HIP_DEVICE_COMPILE__)
        // the piece is consumed from its low end and shifted down a byte at a time: no indexing, so it stays in four registers
        const uint32_t at = p & ~15u;
        if (at != piece_at) {
            piece = *reinterpret_cast<const uint4 *>(base + at);
            piece_at = at;
            for (uint32_t k = p & 15u; k; --k) shift8();       // (only where a segment begins inside a piece)
        }
        const uint32_t b = piece.x & 255u;
        shift8();
        ++p;
        return b;
#else
        return base[p++];
#endif
    }
    Y2J_HD void fill()
    {
        while (n <= 24) {
            uint32_t b = 0;
            if (!dry) {
                b = p < end ? next() : 0;
                if (b == 0xff) {
                    uint32_t c = p < end ? next() : 0;
                    while (c == 0xff) c = p < end ? next() : 0;     // fill bytes (each turn consumes a byte or ends the loop with c == 0)
                    if (c != 0) { marker = (int)c; dry = true; b = 0; }
                }
            }
            acc |= b << (24 - n);
            n += 8;
        }
    }
    Y2J_HD void drop(int k) { acc <<= k; n -= k; }
    Y2J_HD int get(int k)
    {
        if (k == 0) return 0;
        if (n < k) fill();
        const int v = (int)(acc >> (32 - k));
        drop(k);
        return v;
    }
    // the next symbol, or -1 where no code matches
    Y2J_HD int symbol(const Huff &h)
    {
        if (n < 16) fill();
        const uint32_t e = h.look[acc >> 23];
        if (e) { drop((int)(e >> 8)); return (int)(e & 255u); }
        int code = (int)(acc >> 22), len = 10;                       // no code of <= 9 bits matched: at most 7 turns
        for (; len <= 16; ++len, code = (int)(acc >> (32 - len)))
            if (h.maxcode[len] >= 0 && code <= h.maxcode[len] && code >= h.mincode[len]) break;
        if (len > 16) return -1;
        drop(len);
        return h.vals[(h.valptr[len] + code - h.mincode[len]) & 255];
    }
    // RECEIVE + EXTEND (T.81 F.2.2.1), k <= 16
    Y2J_HD int extend(int k)
    {
        if (k == 0) return 0;
        const int v = get(k);
        return v < (1 << (k - 1)) ? v - (1 << k) + 1 : v;
    }
};

// One block: DC difference + AC run/size pairs, dequantised into 16 bits as they are decoded; d (zeroed by the caller) receives the
// coefficients in natural order.  Every turn of the AC loop advances k, so it ends within 63 turns whatever the data.
Y2J_HD inline int block_sequential(Bits &br, const Huff &hd, const Huff &ha, const uint16_t *q, int &dc_pred, int16_t *d)
{
    const int t = br.symbol(hd);
    if (t < 0 || t > 16) return kBadCode;
    dc_pred += br.extend(t);
    d[0] = (int16_t)(dc_pred * q[0]);
    for (int k = 1; k < 64;) {
        const int rs = br.symbol(ha);
        if (rs < 0) return kBadCode;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (rs != 0xf0) break;
            k += 16;
        } else {
            k += r;
            if (k > 63) return kCoefOverrun;
            const int z = zigzag(k++);
            d[z] = (int16_t)(br.extend(s) * q[z]);
        }
    }
    return kOk;
}

// The MCUs of one segment, from a reset reader and zero predictions, into the frame's coefficients (zeroed beforehand), then the restart
// rule: the interval must have ended at RSTn - for the scan's last one, at a marker (the parser made sure which).  The trip counts are
// the geometry's (n_mcu x blocks of an MCU x 64), never the data's.
Y2J_HD inline int decode_segment(const Frame &f, const Tables &t, const uint8_t *streams, const Segment &s, int16_t *coef)
{
    Bits br;
    br.open(streams, s.begin, s.end);
    int pred[3] = {0, 0, 0};
    int mx = s.first_mcu % f.mcu_x, my = s.first_mcu / f.mcu_x;
    for (int m = 0; m < s.n_mcu; ++m) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 3; ++k) {          // pred[] is indexed by scan position: a register each
            if (k >= f.ncomp) break;
            const int ci = f.order[k];
            const Comp &c = f.comp[ci];
            const int bw = c.w2 >> 3;
            for (int y = 0; y < c.v; ++y)
                for (int x = 0; x < c.h; ++x) {
                    const int bx = mx * c.h + x, by = my * c.v + y;
                    const int rc = block_sequential(br, t.dc[ci], t.ac[ci], t.q[ci], pred[k], coef + c.off + ((size_t)by * bw + bx) * 64);
                    if (rc) return rc;
                }
        }
        if (++mx == f.mcu_x) { mx = 0; ++my; }
    }
    if (br.n < 24) br.fill();
    if (s.last ? br.marker < 0 : (br.marker < 0xd0 || br.marker > 0xd7)) return kRestartOutOfStep;
    return kOk;
}

// ---------------------------------------------------------------------------- one segment, many lanes
// A segment's bytes [begin, data_end) - data_end: the first FF of the marker that ends it - are cut into subsequences of `sub` RAW
// bytes; lane i decodes the symbols that START inside subsequence i.  Huffman streams re-synchronise, so a lane started at a boundary
// soon walks the true symbol boundaries; rounds of "decode the next subsequence from my own exit state, stop when the record there is
// what I computed" spread the true state of lane 0 over the segment (split_segment_host below is the whole algorithm as loops; the
// kernel k_jpegdec_split is the same calls with a workgroup's lanes and barriers for the loops).
//
// POSITIONS.  A decoder's place is (off, bit): the raw offset of the first byte of the UNIT that holds the next unread bit, and the bit
// inside it.  A unit is one data byte: a byte that is not FF, or FF.. 00 (a stuffed FF, fill bytes included).  Two decoders that
// reach one bit by different routes report one place, whatever they prefetched: SBits keeps, beside `acc`, the raw length of each of
// the (at most four) units it holds, and its place is `p` minus the lengths of the units not yet used up.  The stream is read in
// place and stays intact.  Price: a register, and a handful of integer operations per symbol for where().
constexpr int kSplitMin = 16, kSplitMax = 4096;   // option jpegdec_split: multiples of 16 in this range
constexpr int kSplitMaxSub = 2048;                // subsequences of one segment (and of one workgroup): the subsequence is doubled until they fit

struct SBits {
    const uint8_t *base;
    uint32_t p, lim;       // next raw byte to fetch; data_end
    uint32_t acc, lens;    // lens: raw length of the last four units fetched, the newest in the low byte (0: a zero byte behind the data)
    int n;
    bool lost;             // a unit longer than 255 bytes, or an FF run that does not end in 00: the lane stops
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 piece;
    uint32_t piece_at;
    __device__ void shift8()
    {
        piece.x = (piece.x >> 8) | (piece.y << 24); piece.y = (piece.y >> 8) | (piece.z << 24);
        piece.z = (piece.z >> 8) | (piece.w << 24); piece.w >>= 8;
    }
#endif
    Y2J_HD uint32_t next()   // as Bits::next
    {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t at = p & ~15u;
        if (at != piece_at) {
            piece = *reinterpret_cast<const uint4 *>(base + at);
            piece_at = at;
            for (uint32_t k = p & 15u; k; --k) shift8();
        }
        const uint32_t b = piece.x & 255u;
        shift8();
        ++p;
        return b;
#else
        return base[p++];
#endif
    }
    Y2J_HD void fill()
    {
        while (n <= 24) {
            uint32_t b = 0, len = 0;
            if (p < lim) {
                b = next();
                len = 1;
                if (b == 0xff) {
                    uint32_t c = 0xff;
                    while (c == 0xff && p < lim) { c = next(); ++len; }      // (bounded by lim)
                    if (c != 0 || len > 255) { lost = true; len = 255; }
                }
            }
            acc |= b << (24 - n);
            n += 8;
            lens = (lens << 8) | len;
        }
    }
    Y2J_HD void drop(int k) { acc <<= k; n -= k; }
    Y2J_HD void open(const uint8_t *b, uint32_t off, int bit, uint32_t data_end)
    {
        base = b; p = off; lim = data_end; acc = 0; lens = 0; n = 0; lost = false;
#if defined(__HIP_DEVICE_COMPILE__)
        piece_at = 0xffffffffu;
        piece = make_uint4(0, 0, 0, 0);
#endif
        if (bit) { fill(); drop(bit); }
    }
    // the place of the next unread bit, and the raw length of the unit that holds it (bit != 0 only)
    Y2J_HD void where(uint32_t &off, int &bit, uint32_t &ulen) const
    {
        const int u = (n + 7) >> 3;
        uint32_t l = lens, sum = 0, last = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; ++i) {
            if (i < u) { last = l & 255u; sum += last; }
            l >>= 8;
        }
        off = p - sum; bit = (8 - (n & 7)) & 7; ulen = last;
    }
    Y2J_HD int get(int k)
    {
        if (k == 0) return 0;
        if (n < k) fill();
        const int v = (int)(acc >> (32 - k));
        drop(k);
        return v;
    }
    Y2J_HD int symbol(const Huff &h)     // Bits::symbol
    {
        if (n < 16) fill();
        const uint32_t e = h.look[acc >> 23];
        if (e) { drop((int)(e >> 8)); return (int)(e & 255u); }
        int code = (int)(acc >> 22), len = 10;
        for (; len <= 16; ++len, code = (int)(acc >> (32 - len)))
            if (h.maxcode[len] >= 0 && code <= h.maxcode[len] && code >= h.mincode[len]) break;
        if (len > 16) return -1;
        drop(len);
        return h.vals[(h.valptr[len] + code - h.mincode[len]) & 255];
    }
    Y2J_HD int extend(int k)
    {
        if (k == 0) return 0;
        const int v = get(k);
        return v < (1 << (k - 1)) ? v - (1 << k) + 1 : v;
    }
};

// What a lane leaves for one subsequence: its exit state - place, slot (the block's index within the MCU) and k (the zigzag index
// expected next, 0: a DC symbol) - and what it decoded on the way: blocks completed, the sum of DC differences per component
// (wrapping, as block_sequential's dc_pred += does), and whether the place behind the LAST block it completed is where a complete
// segment ends.  The whole record is a function of the entry state, and the rounds compare whole records.
struct SplitRec {
    uint32_t off;
    uint32_t meta;      // bit 0..2 | slot << 3 | k << 6 | kSplitStopped | kSplitCloseOk
    uint32_t nblk;
    int32_t dc[3];
};
constexpr uint32_t kSplitStopped = 1u << 12, kSplitCloseOk = 1u << 13, kSplitStateMask = 0xfffu | kSplitStopped;
Y2J_HD inline bool split_same(const SplitRec &a, const SplitRec &b)
{
    return a.off == b.off && a.meta == b.meta && a.nblk == b.nblk && a.dc[0] == b.dc[0] && a.dc[1] == b.dc[1] && a.dc[2] == b.dc[2];
}
// slot -> component | x << 2 | y << 3, four bits a slot (at most 6 slots: luma 2x2 and two chroma blocks); the blocks of an MCU
Y2J_HD inline uint32_t split_slot_map(const Frame &f, int &bpm)
{
    uint32_t m = 0;
    int s = 0;
    for (int k = 0; k < 3; ++k) {
        if (k >= f.ncomp) break;
        const int ci = f.order[k];
        for (int y = 0; y < f.comp[ci].v; ++y)
            for (int x = 0; x < f.comp[ci].h; ++x, ++s) m |= (uint32_t)(ci | (x << 2) | (y << 3)) << (4 * s);
    }
    bpm = s;
    return m;
}

// What the writing pass knows on entry beside the state: the ordinal of the block it is in, the DC predictions, and where blocks go.
struct SplitWrite {
    int ordinal, n_blocks, first_mcu;
    int pred[3];
    int16_t *coef;      // the frame's
};

// The symbols that start in [state's place, sub_end) from the state in (in.off, in.meta); `turns` = 8 * subsequence bytes + 16 bounds
// the loop.  A bad code, k > 63 or a lost reader STOPS the lane (kSplitStopped): on a speculative lane that is no error, the lane
// below overwrites the record; on the true chain it sends the segment to decode_segment unless the geometry's blocks were complete.
// kWrite: the same walk from a verified state, storing what block_sequential stores, for blocks below w.n_blocks only.
template <bool kWrite>
Y2J_HD inline void split_run(const Frame &f, const Tables &t, const uint8_t *base, uint32_t data_end, uint32_t sub_end, uint32_t smap, int bpm,
                             int turns, uint32_t in_off, uint32_t in_meta, SplitRec &out, SplitWrite &w)
{
    SBits br;
    br.open(base, in_off, (int)(in_meta & 7u), data_end);
    int slot = (int)((in_meta >> 3) & 7u), k = (int)((in_meta >> 6) & 63u);
    uint32_t nblk = 0, close_ok = 0, off = in_off, ulen = 0;
    int bit = 0, d0 = 0, d1 = 0, d2 = 0, p0 = 0, p1 = 0, p2 = 0, mx = 0, my = 0;
    int16_t *d = nullptr;
    bool stopped = false;
    auto block_at = [&]() {
        const uint32_t e = smap >> (4 * slot);
        const Comp &c = f.comp[e & 3u];
        const int bx = mx * c.h + (int)((e >> 2) & 1u), by = my * c.v + (int)((e >> 3) & 1u);
        d = w.coef + c.off + ((size_t)by * (size_t)(c.w2 >> 3) + (size_t)bx) * 64;
    };
    if (kWrite) {
        p0 = w.pred[0]; p1 = w.pred[1]; p2 = w.pred[2];
        const int mcu = w.first_mcu + w.ordinal / bpm;
        mx = mcu % f.mcu_x; my = mcu / f.mcu_x;
        block_at();
    }
    int turn = 0;
    for (; turn < turns; ++turn) {
        br.where(off, bit, ulen);
        if (off >= sub_end) break;
        if (kWrite && w.ordinal >= w.n_blocks) break;
        if (br.lost) { stopped = true; break; }
        const int ci = (int)((smap >> (4 * slot)) & 3u);
        if (k == 0) {
            const int s = br.symbol(t.dc[ci]);
            if (s < 0 || s > 16) { stopped = true; break; }
            const int diff = br.extend(s);
            if (ci == 0) d0 += diff; else if (ci == 1) d1 += diff; else d2 += diff;
            if (kWrite) {
                int pred;
                if (ci == 0) pred = (p0 += diff); else if (ci == 1) pred = (p1 += diff); else pred = (p2 += diff);
                d[0] = (int16_t)(pred * t.q[ci][0]);
            }
            k = 1;
        } else {
            const int rs = br.symbol(t.ac[ci]);
            if (rs < 0) { stopped = true; break; }
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                k = rs == 0xf0 ? k + 16 : 64;
            } else {
                k += r;
                if (k > 63) { stopped = true; break; }
                const int z = zigzag(k++);
                const int v = br.extend(s);
                if (kWrite) d[z] = (int16_t)(v * t.q[ci][z]);
            }
        }
        if (k >= 64) {
            k = 0;
            ++nblk;
            if (++slot == bpm) {
                slot = 0;
                if (kWrite && ++mx == f.mcu_x) { mx = 0; ++my; }
            }
            br.where(off, bit, ulen);
            close_ok = (bit ? off + ulen : off) == data_end ? kSplitCloseOk : 0u;
            if (kWrite) { ++w.ordinal; block_at(); }
        }
    }
    if (turn == turns || br.lost) stopped = true;
    out.nblk = nblk; out.dc[0] = d0; out.dc[1] = d1; out.dc[2] = d2;
    if (stopped) { out.off = 0xffffffffu; out.meta = kSplitStopped | close_ok; }
    else { out.off = off; out.meta = (uint32_t)bit | ((uint32_t)slot << 3) | ((uint32_t)k << 6) | close_ok; }
}

// How one lane reads the scanned records: `before` = the exclusive prefix over the segment's subsequences in front of it (blocks, DC
// sums, and whether any of them stopped), `own` = its record.  n_blocks = n_mcu x blocks of an MCU.  The segment is ACCEPTED when
// some lane closes it and no lane overshoots; everything else is decode_segment's.
//   closes:     on the true chain, the geometry's last block is completed here, and behind it less than one unit of data is left in
//               front of the marker - where decode_segment's closing rule finds the marker whatever its reader had prefetched;
//   overshoots: on the true chain and its blocks go past the geometry's (pad bits that decode into blocks, or damage).
Y2J_HD inline bool split_closes(uint32_t before_nblk, bool before_stopped, const SplitRec &own, uint32_t n_blocks)
{
    return !before_stopped && before_nblk < n_blocks && before_nblk + own.nblk == n_blocks && (own.meta & kSplitCloseOk);
}
Y2J_HD inline bool split_overshoots(uint32_t before_nblk, bool before_stopped, const SplitRec &own, uint32_t n_blocks)
{
    return !before_stopped && before_nblk + own.nblk > n_blocks;
}

Y2J_HD constexpr int fx12(float x) { return (int)(x * 4096 + 0.5); }

// One 1-D pass of the inverse DCT (idct_1d of y2_codec.cpp): outputs are x0 +- t3, x1 +- t2, x2 +- t1, x3 +- t0, scaled by 4096.
Y2J_HD inline void idct_1d(int s0, int s1, int s2, int s3, int s4, int s5, int s6, int s7, int x[4], int t[4])
{
    int p2 = s2, p3 = s6;
    int p1 = (p2 + p3) * fx12(0.5411961f);
    const int e2 = p1 + p3 * fx12(-1.847759065f), e3 = p1 + p2 * fx12(0.765366865f);
    p2 = s0; p3 = s4;
    const int e0 = (p2 + p3) * 4096, e1 = (p2 - p3) * 4096;
    x[0] = e0 + e3; x[3] = e0 - e3; x[1] = e1 + e2; x[2] = e1 - e2;
    int t0 = s7, t1 = s5, t2 = s3, t3 = s1;
    p3 = t0 + t2;
    int p4 = t1 + t3;
    p1 = t0 + t3;
    p2 = t1 + t2;
    const int p5 = (p3 + p4) * fx12(1.175875602f);
    t0 *= fx12(0.298631336f); t1 *= fx12(2.053119869f); t2 *= fx12(3.072711026f); t3 *= fx12(1.501321110f);
    p1 = p5 + p1 * fx12(-0.899976223f);
    p2 = p5 + p2 * fx12(-2.562915447f);
    p3 *= fx12(-1.961570560f);
    p4 *= fx12(-0.390180644f);
    t[3] = t3 + p1 + p4; t[2] = t2 + p2 + p3; t[1] = t1 + p2 + p4; t[0] = t0 + p1 + p3;
}

Y2J_HD inline uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// stb's islow arithmetic: columns with +512 >> 10, rows with +65536 + (128 << 17) >> 17, clamped.  Every index is a constant once
// the loops are unrolled, so v[] lives in registers on the device.
Y2J_HD inline void idct_block(uint8_t *out, int stride, const int16_t *d)
{
    int v[64];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) {
        int x[4], t[4];
        idct_1d(d[c], d[c + 8], d[c + 16], d[c + 24], d[c + 32], d[c + 40], d[c + 48], d[c + 56], x, t);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k) {
            const int e = x[k] + 512;
            v[k * 8 + c] = (e + t[3 - k]) >> 10;
            v[(7 - k) * 8 + c] = (e - t[3 - k]) >> 10;
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; ++r) {
        int x[4], t[4];
        idct_1d(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7], x, t);
        uint8_t o[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k) {
            const int e = x[k] + 65536 + (128 << 17);
            o[k] = clamp255((e + t[3 - k]) >> 17);
            o[7 - k] = clamp255((e - t[3 - k]) >> 17);
        }
        uint8_t *row = out + (size_t)r * stride;     // plane rows are multiples of 8 samples from an aligned base: two aligned words
        reinterpret_cast<uint32_t *>(row)[0] = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
        reinterpret_cast<uint32_t *>(row)[1] = (uint32_t)o[4] | ((uint32_t)o[5] << 8) | ((uint32_t)o[6] << 16) | ((uint32_t)o[7] << 24);
    }
}

// Sample (x, y) of the full-size picture from one component's plane: row_1 / row_v2 / row_h2 / row_hv2 of y2_codec.cpp as functions of
// the output position (hs, vs in {1, 2}; wl = ceil(width / hs) samples take part, cy = the component's effective rows).
Y2J_HD inline int up_sample(const uint8_t *pl, int w2, int cy, int hs, int vs, int wl, int x, int y)
{
    const uint8_t *near = pl + (size_t)y * w2, *far = near;
    if (vs == 2) {
        const int k = y >> 1, fr = (y & 1) ? (k + 1 < cy ? k + 1 : cy - 1) : (k > 0 ? k - 1 : 0);
        near = pl + (size_t)k * w2;
        far = pl + (size_t)fr * w2;
    }
    if (hs == 1) return vs == 1 ? near[x] : (3 * near[x] + far[x] + 2) >> 2;
    const int i = x >> 1;
    if (vs == 1) {
        if (wl == 1) return near[0];
        if (x & 1) return i == wl - 1 ? near[wl - 1] : (3 * near[i] + near[i + 1] + 2) >> 2;
        if (i == 0) return near[0];
        if (i == wl - 1) return (near[wl - 2] * 3 + near[wl - 1] + 2) >> 2;     // (the reference's last pair: weights on w-2, w-1)
        return (3 * near[i] + near[i - 1] + 2) >> 2;
    }
    const int ti = 3 * near[i] + far[i];
    if (wl == 1) return (ti + 2) >> 2;
    if (x & 1) return i == wl - 1 ? (ti + 2) >> 2 : (3 * ti + (3 * near[i + 1] + far[i + 1]) + 8) >> 4;
    return i == 0 ? (ti + 2) >> 2 : (3 * ti + (3 * near[i - 1] + far[i - 1]) + 8) >> 4;
}

Y2J_HD constexpr int fx20(float x) { return ((int)(x * 4096.0f + 0.5f)) << 8; }

// YCbCr -> RGB in 20-bit fixed point; green keeps the & 0xffff0000 of its Cb term
Y2J_HD inline void ycc_to_rgb(uint8_t *out, int y, int cb, int cr)
{
    const int yf = (y << 20) + (1 << 19);
    cr -= 128; cb -= 128;
    const int r = (yf + cr * fx20(1.40200f)) >> 20;
    const int g = (int)(yf + cr * -fx20(0.71414f) + (int)((unsigned)(cb * -fx20(0.34414f)) & 0xffff0000u)) >> 20;
    const int b = (yf + cb * fx20(1.77200f)) >> 20;
    out[0] = clamp255(r); out[1] = clamp255(g); out[2] = clamp255(b);
}

// RGB24 of output pixel (x, y) from the frame's planes (one component: its sample three times)
Y2J_HD inline void rgb_pixel(const Frame &f, const uint8_t *planes, int x, int y, uint8_t out[3])
{
    int s[3] = {0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        if (k >= f.ncomp) break;
        const Comp &c = f.comp[k];
        const int hs = f.hmax / c.h, vs = f.vmax / c.v;
        s[k] = up_sample(planes + c.off, c.w2, c.y, hs, vs, (f.width + hs - 1) / hs, x, y);
    }
    if (f.ncomp == 1) out[0] = out[1] = out[2] = (uint8_t)s[0];
    else ycc_to_rgb(out, s[0], s[1], s[2]);
}

}  // namespace y2jpg
