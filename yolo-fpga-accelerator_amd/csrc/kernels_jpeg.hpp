// kernels_jpeg.hpp -- RGB24 frames in HBM -> the JPEG streams the reference's MJPEG streamer sends for them (stb_image_write v1.09,
// 3 components, no subsampling; host/y2_jpeg.cpp is the same encoder on the host and the expected side of the tests), byte for byte.
//
// A sequential encoder carries two things from block to block: the DC predictor and the bit position.  Here the first is a look at
// the coefficients of the MCU before, and the second a prefix sum, so every stage is parallel over blocks.  Stages are separate
// launches and the kernel boundary is the only hand-off between workgroups; the only atomics are integer ORs, so the bytes do not
// depend on arrival order.  A block is one (MCU, component) pair, in stream order: block b = 3 * mcu + component.
//   k_jpeg_transform   A   a lane per block: pixels (edge pixels repeated) -> colour transform -> AAN row and column passes in
//                          registers -> times fdtbl, rounded, in zigzag order -> int16 coef[block][64].  Every fp32 operation is
//                          rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn) in the reference's order: one fused
//                          multiply-add changes bytes.
//   k_jpeg_lengths     B   a lane per block: the block's bit count from its coefficients and the DC of block b - 3; exclusive scan
//                          within the workgroup of kJpegBlocks blocks -> blk_off, the workgroup's total -> wg_sum
//   k_jpeg_scan_groups B   a workgroup per frame: exclusive scan of wg_sum -> wg_base (64-bit bit offsets), the frame's bit and
//                          byte totals; zeroes the two dwords of the unstuffed stream at every group's ends
//   k_jpeg_pack        C   a workgroup per kJpegBlocks blocks: code words ORed into an LDS image of the group's bit range, then
//                          whole dwords stored and the (at most two) dwords shared with the neighbours atomicOr-ed; the frame's
//                          last group fills the last partial byte with ones
//   k_jpeg_count_ff    D   0xFF bytes per kJpegSegBytes segment of the unstuffed stream
//   k_jpeg_scan_segs   D   a workgroup per frame: exclusive scan of the segment counts, the stream's size
//   k_jpeg_place       D   one workgroup: where each frame's stream starts in the packed output (sum of min(size, capacity))
//   k_jpeg_emit        D   header, stuffed bytes (a zero after every 0xFF) and FF D9, nothing at or beyond the frame's capacity
// The tables (fdtbl, code words, header) come from csrc/jpeg_tables.hpp on the host and lead the chunk's table.  Stages B, C and the
// emit kernel are templates: <false> is the above; <true> ("optimize" at the end of this file) takes the code words and the header
// from the frame's JpegOptFrame.
//
// Launched from yolo2_jpeg.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_tables.hpp"

namespace y2 {

// The table that leads a chunk (AnnoHeader / AnnoFrame lead the painter's the same way): the tables, then one JpegFrame per frame.
struct JpegHeader {
    y2j::Tables t;
};
struct JpegFrame {
    unsigned long long src_off;   // the frame's RGB24 bytes, from the source base address
    unsigned long long us_off;    // its unstuffed stream in the work area, bytes (a multiple of 256), room for blocks * kBlockBitsMax bits
    unsigned long long cap;       // bytes the caller has room for: nothing at or beyond it is written
    int w, h, mcux;               // mcux: MCUs per row
    int n_blk;                    // 3 * MCUs (6 * MCUs with subsample 420)
    int subsample, restart;       // the mode (jpeg_tables.hpp); (0, 0): the reference's stream
    unsigned n_int, rst0;         // its intervals (1 without restart) and where they start in rst_off
    unsigned blk0;                // its first block in coef / blk_off
    unsigned wg0, n_wg;           // its groups of kJpegBlocks blocks in wg_sum / wg_base
    unsigned seg0;                // its segments in seg_ff / seg_base (room for the bound)
};
// what the stages leave per frame
struct JpegState {
    unsigned long long bits;      // the scan before the fill
    unsigned long long ubytes;    // ceil(bits / 8): the unstuffed scan
    unsigned long long ff;        // 0xFF bytes in it
    unsigned long long size;      // kHeaderBytes + ubytes + ff + 2
    unsigned long long out_off;   // where the stream starts in the packed output
};

// optimize = 1 (jpeg_opt.hpp): what k_jpeg_opt_tables leaves per frame for the <true> forms of stages B, C and D
struct JpegOptFrame {
    uint32_t code[4][256];                  // the frame's code words, or Tables::code where it falls back
    uint32_t head_len, used;                // the header's bytes; 1: the frame's own tables
    uint8_t header[y2j::kOptHeaderSlot];    // the frame's header, size and sampling in place
};

constexpr int kJpegBlocks = 128;      // blocks (= lanes) per workgroup of stages A, B and C
constexpr int kJpegScan = 256;        // lanes of the per-frame scans
constexpr int kJpegSegBytes = 4096;   // unstuffed bytes per segment of stage D: 256 lanes of 16 bytes
constexpr int kJpegSegThreads = 256;
// a group's bit range in LDS: up to 31 bits of the neighbour before it, its blocks, up to 7 fill bits, and one dword of slack that
// jpeg_put's second OR and the zeroing loop may touch
constexpr int kJpegPackDwords = (31 + kJpegBlocks * y2j::kBlockBitsMax + 7 + 31) / 32 + 1;

__device__ inline const JpegFrame &jpeg_frame(const uint8_t *table, int f)
{
    return reinterpret_cast<const JpegFrame *>(table + sizeof(JpegHeader))[f];
}

// inclusive scan of one value per lane over a workgroup of N lanes (N a power of two), through s[N]
template <int N>
__device__ inline uint32_t jpeg_scan_incl(uint32_t v, uint32_t *s, int tid)
{
    s[tid] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < N; d <<= 1) {
        const uint32_t t = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    return s[tid];
}

// ---------------------------------------------------------------------------------------------------------------- A: transform

// one 8-point AAN pass (host/y2_jpeg.cpp aan_pass, operation for operation)
__device__ inline void jpeg_aan(float &d0, float &d1, float &d2, float &d3, float &d4, float &d5, float &d6, float &d7)
{
    const float a0 = __fadd_rn(d0, d7), a7 = __fsub_rn(d0, d7), a1 = __fadd_rn(d1, d6), a6 = __fsub_rn(d1, d6);
    const float a2 = __fadd_rn(d2, d5), a5 = __fsub_rn(d2, d5), a3 = __fadd_rn(d3, d4), a4 = __fsub_rn(d3, d4);
    const float e0 = __fadd_rn(a0, a3), e3 = __fsub_rn(a0, a3), e1 = __fadd_rn(a1, a2), e2 = __fsub_rn(a1, a2);
    d0 = __fadd_rn(e0, e1);
    d4 = __fsub_rn(e0, e1);
    const float r = __fmul_rn(__fadd_rn(e2, e3), 0.707106781f);
    d2 = __fadd_rn(e3, r);
    d6 = __fsub_rn(e3, r);
    const float o0 = __fadd_rn(a4, a5), o1 = __fadd_rn(a5, a6), o2 = __fadd_rn(a6, a7);
    const float k = __fmul_rn(__fsub_rn(o0, o2), 0.382683433f);
    const float p = __fadd_rn(__fmul_rn(o0, 0.541196100f), k), q = __fadd_rn(__fmul_rn(o2, 1.306562965f), k), m = __fmul_rn(o1, 0.707106781f);
    const float s0 = __fadd_rn(a7, m), s1 = __fsub_rn(a7, m);
    d5 = __fadd_rn(s1, p);
    d3 = __fsub_rn(s1, p);
    d1 = __fadd_rn(s0, q);
    d7 = __fsub_rn(s0, q);
}

// grid (ceil(max n_blk / kJpegBlocks), frames)
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_transform(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                                int16_t *__restrict__ coef)
{
    __shared__ float s_fd[2][64];
    const JpegHeader *hd = reinterpret_cast<const JpegHeader *>(table);
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x * kJpegBlocks >= fr.n_blk) return;   // (the whole workgroup)
    s_fd[tid >> 6][tid & 63] = hd->t.fdtbl[tid >> 6][tid & 63];
    __syncthreads();
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    if (b >= fr.n_blk) return;
    const int mcu = b / 3, comp = b - mcu * 3;
    const int my = mcu / fr.mcux, mx = mcu - my * fr.mcux;
    // Y = .299 r + .587 g + .114 b - 128, U = -.16874 r - .33126 g + .5 b, V = .5 r - .41869 g - .08131 b, each left to right; a
    // subtraction of a product is the addition of the product with the negated constant, bit for bit
    const float c0 = comp == 0 ? 0.299f : comp == 1 ? -0.16874f : 0.5f;
    const float c1 = comp == 0 ? 0.587f : comp == 1 ? -0.33126f : -0.41869f;
    const float c2 = comp == 0 ? 0.114f : comp == 1 ? 0.5f : -0.08131f;
    const uint8_t *src = src_base + fr.src_off;
    float d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint8_t *row = src + (size_t)min(my * 8 + r, fr.h - 1) * fr.w * 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint8_t *px = row + (size_t)min(mx * 8 + c, fr.w - 1) * 3;
            const float R = (float)px[0], G = (float)px[1], B = (float)px[2];
            float v = __fadd_rn(__fadd_rn(__fmul_rn(c0, R), __fmul_rn(c1, G)), __fmul_rn(c2, B));
            if (comp == 0) v = __fsub_rn(v, 128.f);
            d[r * 8 + c] = v;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) jpeg_aan(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5], d[8 * r + 6], d[8 * r + 7]);
#pragma unroll
    for (int c = 0; c < 8; ++c) jpeg_aan(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
    const float *fd = s_fd[comp != 0];
    uint32_t pk[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) pk[i] = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const float v = __fmul_rn(d[i], fd[i]);
        const int q = (int)(v < 0.f ? __fsub_rn(v, 0.5f) : __fadd_rn(v, 0.5f));
        const int z = y2j::kZigzag[i];
        pk[z >> 1] |= ((uint32_t)q & 0xffffu) << (16 * (z & 1));
    }
    uint4 *o = reinterpret_cast<uint4 *>(coef + ((size_t)fr.blk0 + b) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = make_uint4(pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]);
}

// ---------------------------------------------------------------------------------------------------------------- B: lengths

__device__ inline int jpeg_category(int v) { return 32 - __clz(v < 0 ? -v : v); }   // bits of |v|; 0 for 0

// a block's coefficients (zigzag order), two per dword
struct JpegBlock {
    uint32_t pk[32];
    __device__ inline void load(const int16_t *coef, size_t blk)
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(coef + blk * 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 v = p[i];
            pk[4 * i] = v.x; pk[4 * i + 1] = v.y; pk[4 * i + 2] = v.z; pk[4 * i + 3] = v.w;
        }
    }
    __device__ inline int at(int i) const { return (int)(int16_t)(pk[i >> 1] >> (16 * (i & 1))); }   // (i is a constant after unrolling)
};

// the code words into LDS: the chunk's (kOpt false: opt is not read), or the frame's own
template <bool kOpt>
__device__ inline void jpeg_stage_codes(uint32_t *s_code, const uint8_t *table, const JpegOptFrame *opt, int frame, int tid, int threads)
{
    const uint32_t *code = kOpt ? &opt[frame].code[0][0] : &reinterpret_cast<const JpegHeader *>(table)->t.code[0][0];
    for (int i = tid; i < 4 * 256; i += threads) s_code[i] = code[i];
}
// the DC predictor of block blk: the DC level `back` blocks before it, zero for back = 0 (stages B and C and k_jpeg_hist)
__device__ inline int jpeg_dc_pred(const int16_t *coef, size_t blk, int back) { return back ? (int)coef[(blk - back) * 64] : 0; }

// grid (ceil(max n_blk / kJpegBlocks), frames)
template <bool kOpt>
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_lengths(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                              uint32_t *__restrict__ blk_off, uint32_t *__restrict__ wg_sum,
                                                              const JpegOptFrame *__restrict__ opt)
{
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint32_t s_scan[kJpegBlocks];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    jpeg_stage_codes<kOpt>(s_code, table, opt, blockIdx.y, tid, kJpegBlocks);
    __syncthreads();
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    uint32_t bits = 0;
    if (b < fr.n_blk) {
        const size_t blk = (size_t)fr.blk0 + b;
        const uint32_t *dc = s_code + (b % 3 ? 2 : 0) * 256, *ac = dc + 256;
        JpegBlock c;
        c.load(coef, blk);
        const int pred = jpeg_dc_pred(coef, blk, b >= 3 ? 3 : 0);
        const int cat = jpeg_category(c.at(0) - pred);
        bits = (dc[cat] >> 16) + cat;
        int run = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int v = c.at(i);
            if (v == 0) {
                ++run;
            } else {
                const int k = jpeg_category(v);
                bits += (run >> 4) * (ac[0xF0] >> 16) + (ac[((run & 15) << 4) | k] >> 16) + k;
                run = 0;
            }
        }
        if (run) bits += ac[0] >> 16;
    }
    const uint32_t incl = jpeg_scan_incl<kJpegBlocks>(bits, s_scan, tid);
    if (b < fr.n_blk) blk_off[(size_t)fr.blk0 + b] = incl - bits;
    if (tid == kJpegBlocks - 1) wg_sum[fr.wg0 + blockIdx.x] = incl;
}

// grid (frames): wg_sum -> wg_base, the frame's totals; the stream's dwords at every group's two ends are zeroed for k_jpeg_pack's ORs
__global__ __launch_bounds__(kJpegScan) void k_jpeg_scan_groups(const uint8_t *__restrict__ table, const uint32_t *__restrict__ wg_sum,
                                                                unsigned long long *__restrict__ wg_base, uint8_t *__restrict__ us_base,
                                                                JpegState *__restrict__ state)
{
    __shared__ uint32_t s_scan[kJpegScan];
    const JpegFrame fr = jpeg_frame(table, blockIdx.x);
    const int tid = threadIdx.x;
    uint32_t *us = reinterpret_cast<uint32_t *>(us_base + fr.us_off);
    unsigned long long running = 0;
    for (unsigned base = 0; base < fr.n_wg; base += kJpegScan) {
        const unsigned i = base + tid;
        const uint32_t v = i < fr.n_wg ? wg_sum[fr.wg0 + i] : 0u;
        const uint32_t incl = jpeg_scan_incl<kJpegScan>(v, s_scan, tid);
        if (i < fr.n_wg) {
            const unsigned long long lo = running + (incl - v), hi = lo + v;   // (v > 0: a block has at least a DC code and an end-of-block)
            wg_base[fr.wg0 + i] = lo;
            us[lo >> 5] = 0u;
            us[(hi - 1) >> 5] = 0u;
        }
        running += s_scan[kJpegScan - 1];
        __syncthreads();
    }
    if (tid == 0) {
        state[blockIdx.x].bits = running;
        state[blockIdx.x].ubytes = (running + 7) >> 3;
    }
}

// ---------------------------------------------------------------------------------------------------------------- C: bits

// n <= 26 bits of v, most significant first, at bit `pos` of the LDS image (bit 0 is the top bit of dword 0)
__device__ inline void jpeg_put(uint32_t *s_bits, uint32_t &pos, uint32_t v, int n)
{
    const uint64_t x = (uint64_t)v << (64 - (int)(pos & 31u) - n);
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    atomicOr(&s_bits[pos >> 5], hi);
    if (lo) atomicOr(&s_bits[(pos >> 5) + 1], lo);
    pos += (uint32_t)n;
}
__device__ inline uint32_t jpeg_extra(int v, int cat) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u); }

// grid (ceil(max n_blk / kJpegBlocks), frames)
template <bool kOpt>
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_pack(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                           const uint32_t *__restrict__ blk_off, const uint32_t *__restrict__ wg_sum,
                                                           const unsigned long long *__restrict__ wg_base, uint8_t *__restrict__ us_base,
                                                           const JpegOptFrame *__restrict__ opt)
{
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint32_t s_bits[kJpegPackDwords];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    jpeg_stage_codes<kOpt>(s_code, table, opt, blockIdx.y, tid, kJpegBlocks);
    const unsigned long long lo = wg_base[fr.wg0 + blockIdx.x], hi = lo + wg_sum[fr.wg0 + blockIdx.x];
    // the frame's last group also owns the ones that fill the last byte
    const int fill = blockIdx.x + 1 == fr.n_wg ? (int)((8 - (hi & 7)) & 7) : 0;
    const unsigned long long end = hi + fill, d0 = lo >> 5;
    const int nd = (int)(((end - 1) >> 5) - d0) + 1;
    for (int j = tid; j < nd + 1; j += kJpegBlocks) s_bits[j] = 0u;
    __syncthreads();
    const uint32_t first = (uint32_t)(lo - (d0 << 5));   // the group's first bit in the image
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    if (b < fr.n_blk) {
        const size_t blk = (size_t)fr.blk0 + b;
        const uint32_t *dc = s_code + (b % 3 ? 2 : 0) * 256, *ac = dc + 256;
        JpegBlock c;
        c.load(coef, blk);
        uint32_t pos = first + blk_off[blk];
        const int pred = jpeg_dc_pred(coef, blk, b >= 3 ? 3 : 0);
        const int diff = c.at(0) - pred, cat = jpeg_category(diff);
        jpeg_put(s_bits, pos, ((dc[cat] & 0xffffu) << cat) | jpeg_extra(diff, cat), (int)(dc[cat] >> 16) + cat);
        int run = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int v = c.at(i);
            if (v == 0) {
                ++run;
            } else {
                for (; run >= 16; run -= 16) jpeg_put(s_bits, pos, ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));
                const int k = jpeg_category(v);
                const uint32_t cw = ac[(run << 4) | k];
                jpeg_put(s_bits, pos, ((cw & 0xffffu) << k) | jpeg_extra(v, k), (int)(cw >> 16) + k);
                run = 0;
            }
        }
        if (run) jpeg_put(s_bits, pos, ac[0] & 0xffffu, (int)(ac[0] >> 16));
    }
    if (tid == 0 && fill) {
        uint32_t pos = (uint32_t)(hi - (d0 << 5));
        jpeg_put(s_bits, pos, (1u << fill) - 1u, fill);
    }
    __syncthreads();
    // the stream is bytes, most significant bit first: the image's dwords go out byte-swapped
    uint32_t *us = reinterpret_cast<uint32_t *>(us_base + fr.us_off);
    for (int j = tid; j < nd; j += kJpegBlocks) {
        const unsigned long long g = d0 + j;
        const uint32_t v = __builtin_bswap32(s_bits[j]);
        if ((g << 5) >= lo && ((g + 1) << 5) <= hi) us[g] = v;   // all 32 bits are this group's
        else atomicOr(&us[g], v);                                 // shared with a neighbour (or the frame's last, partial dword): zeroed by k_jpeg_scan_groups
    }
}

// ---------------------------------------------------------------------------------------------------------------- D: stuffing

// the 16 bytes of lane `tid` of segment `seg`: how many are 0xFF (bytes at or beyond ubytes do not count)
__device__ inline int jpeg_seg_load(const uint8_t *us, unsigned long long ubytes, unsigned long long at, uint32_t w[4])
{
    int ff = 0;
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (at < ubytes) {
        const uint4 v = *reinterpret_cast<const uint4 *>(us + at);   // (the work area has room for whole 16-byte lines)
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#pragma unroll
        for (int i = 0; i < 16; ++i) ff += at + i < ubytes && ((w[i >> 2] >> (8 * (i & 3))) & 255u) == 255u;
    }
    return ff;
}

// grid (some, frames); a workgroup takes segments blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(kJpegSegThreads) void k_jpeg_count_ff(const uint8_t *__restrict__ table, const uint8_t *__restrict__ us_base,
                                                                   const JpegState *__restrict__ state, uint32_t *__restrict__ seg_ff)
{
    __shared__ uint32_t s_scan[kJpegSegThreads];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    const unsigned long long ubytes = state[blockIdx.y].ubytes;
    const unsigned nseg = (unsigned)((ubytes + kJpegSegBytes - 1) / kJpegSegBytes);
    const int tid = threadIdx.x;
    for (unsigned seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        uint32_t w[4];
        const int ff = jpeg_seg_load(us_base + fr.us_off, ubytes, (unsigned long long)seg * kJpegSegBytes + tid * 16, w);
        const uint32_t incl = jpeg_scan_incl<kJpegSegThreads>((uint32_t)ff, s_scan, tid);
        if (tid == kJpegSegThreads - 1) seg_ff[fr.seg0 + seg] = incl;
        __syncthreads();
    }
}

// grid (frames)
__global__ __launch_bounds__(kJpegScan) void k_jpeg_scan_segs(const uint8_t *__restrict__ table, const uint32_t *__restrict__ seg_ff,
                                                              uint32_t *__restrict__ seg_base, JpegState *__restrict__ state,
                                                              unsigned long long *__restrict__ sizes)
{
    __shared__ uint32_t s_scan[kJpegScan];
    const JpegFrame fr = jpeg_frame(table, blockIdx.x);
    const unsigned long long ubytes = state[blockIdx.x].ubytes;
    const unsigned nseg = (unsigned)((ubytes + kJpegSegBytes - 1) / kJpegSegBytes);
    const int tid = threadIdx.x;
    unsigned long long running = 0;
    for (unsigned base = 0; base < nseg; base += kJpegScan) {
        const unsigned i = base + tid;
        const uint32_t v = i < nseg ? seg_ff[fr.seg0 + i] : 0u;
        const uint32_t incl = jpeg_scan_incl<kJpegScan>(v, s_scan, tid);
        if (i < nseg) seg_base[fr.seg0 + i] = (uint32_t)running + (incl - v);   // (the entries refuse frames whose bound passes 2^31)
        running += s_scan[kJpegScan - 1];
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned long long size = (unsigned long long)y2j::kHeaderBytes + ubytes + running + 2;
        state[blockIdx.x].ff = running;
        state[blockIdx.x].size = size;
        sizes[blockIdx.x] = size;
    }
}

// grid (1): frame f's stream starts where the frames before it end, each cut at its capacity
__global__ __launch_bounds__(kJpegScan) void k_jpeg_place(const uint8_t *__restrict__ table, JpegState *__restrict__ state, int nf)
{
    __shared__ unsigned long long s_sum[kJpegScan];
    const int tid = threadIdx.x;
    unsigned long long running = 0;
    for (int base = 0; base < nf; base += kJpegScan) {
        const int f = base + tid;
        unsigned long long v = 0;
        if (f < nf) {
            const unsigned long long cap = jpeg_frame(table, f).cap;
            v = state[f].size < cap ? state[f].size : cap;
        }
        s_sum[tid] = v;
        __syncthreads();
        for (int d = 1; d < kJpegScan; d <<= 1) {
            const unsigned long long t = tid >= d ? s_sum[tid - d] : 0ull;
            __syncthreads();
            s_sum[tid] += t;
            __syncthreads();
        }
        if (f < nf) state[f].out_off = running + s_sum[tid] - v;
        running += s_sum[kJpegScan - 1];
        __syncthreads();
    }
}

// grid (some, frames), as k_jpeg_count_ff
template <bool kOpt>
__global__ __launch_bounds__(kJpegSegThreads) void k_jpeg_emit(const uint8_t *__restrict__ table, const uint8_t *__restrict__ us_base,
                                                               const JpegState *__restrict__ state, const uint32_t *__restrict__ seg_base,
                                                               uint8_t *__restrict__ out_base, const JpegOptFrame *__restrict__ opt)
{
    __shared__ uint32_t s_scan[kJpegSegThreads];
    const JpegHeader *hd = reinterpret_cast<const JpegHeader *>(table);
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    const JpegState st = state[blockIdx.y];
    uint8_t *out = out_base + st.out_off;
    const int tid = threadIdx.x;
    const int head = kOpt ? (int)opt[blockIdx.y].head_len : y2j::kHeaderBytes;
    if (blockIdx.x == 0) {
        for (int i = tid; i < head; i += kJpegSegThreads) {
            uint8_t v = kOpt ? opt[blockIdx.y].header[i] : hd->t.header[i];
            if (!kOpt) {
                if (i == y2j::kHeaderHeightAt) v = (uint8_t)(fr.h >> 8);
                if (i == y2j::kHeaderHeightAt + 1) v = (uint8_t)fr.h;
                if (i == y2j::kHeaderWidthAt) v = (uint8_t)(fr.w >> 8);
                if (i == y2j::kHeaderWidthAt + 1) v = (uint8_t)fr.w;
            }
            if ((unsigned long long)i < fr.cap) out[i] = v;
        }
        if (tid < 2 && st.size - 2 + tid < fr.cap) out[st.size - 2 + tid] = tid ? 0xD9 : 0xFF;   // EOI
    }
    const unsigned nseg = (unsigned)((st.ubytes + kJpegSegBytes - 1) / kJpegSegBytes);
    for (unsigned seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        uint32_t w[4];
        const unsigned long long at = (unsigned long long)seg * kJpegSegBytes + tid * 16;
        const int ff = jpeg_seg_load(us_base + fr.us_off, st.ubytes, at, w);
        const uint32_t incl = jpeg_scan_incl<kJpegSegThreads>((uint32_t)ff, s_scan, tid);
        unsigned long long o = (unsigned long long)head + at + seg_base[fr.seg0 + seg] + (incl - (uint32_t)ff);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint8_t v = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            if (at + i < st.ubytes) {
                if (o < fr.cap) out[o] = v;
                ++o;
                if (v == 255) {
                    if (o < fr.cap) out[o] = 0;
                    ++o;
                }
            }
        }
        __syncthreads();
    }
}

// ================================================================================================ the modes (jpeg_tables.hpp)
//
// subsample = 420 and restart = R run kernels of their own; mode (0, 0) runs the eight launches above and nothing below.  A block is
// still one lane of stages B and C, in stream order: block b = bpm * mcu + k, bpm = 3 or 6 blocks per MCU.
//   k_jpeg_transform420  A   a workgroup owns kJpeg420Mcus whole MCUs: their RGB bytes go into LDS once (every pixel is fetched once
//                            per workgroup, not once per component), then wavefront k takes block place k of every MCU - Y00 Y01 Y10
//                            Y11 from 8 x 8 pixels, Cb and Cr from the 2 x 2 means of 16 x 16.  (subsample 0 keeps k_jpeg_transform.)
//   k_jpeg_lengths_rst   B   the DC predictor is the previous block of the component (dc_pred_back), zero in an interval's first MCU.
//                            The bit position is no prefix sum any more: an interval's end rounds it up to a byte.  ONE scan with an
//                            associative operator does it: a run of blocks is the function p -> seen ? ceil8(p + pre) + post : p + pre
//                            of the position p it starts at (pre: bits up to its first interval end, post: bits behind that end, whose
//                            later roundings do not depend on p because they start from a multiple of 8), and two runs compose to a run
//                            (JpegRun).  Exclusive scan within the workgroup -> blk_off (pre) / blk_post (post, seen in bit 31); the
//                            group's run -> wg_sum / wg_post.  R = 1 (many ends per group) and an interval that spans groups and scan
//                            rounds are the same operator.
//   k_jpeg_scan_groups_rst B the same scan over the groups' runs in 64 bits -> wg_base, totals; zeroes the groups' end dwords
//   k_jpeg_pack_rst      C   as k_jpeg_pack; the lane of a block that ends an interval (or the scan) fills its last byte with ones,
//                            the lane of a block that starts one leaves rst_off[interval], the interval's byte offset in the
//                            unstuffed stream.  Markers stay out of that stream, so k_jpeg_count_ff / _scan_segs run as they are.
//   k_jpeg_sizes_rst     D   adds DRI and the markers' bytes to the sizes k_jpeg_scan_segs left
//   k_jpeg_emit_rst      D   an entropy byte goes to header + its offset + stuffed zeros before it + 2 * intervals completed before
//                            it; the lane of an interval's first byte writes FF Dn in front of it.  The interval of a byte: one
//                            binary search per segment for the intervals its two ends lie in, one per lane inside that range, then
//                            a step per interval start passed.

constexpr int kJpeg420Mcus = 64;                    // MCUs per workgroup of k_jpeg_transform420: one per lane of a wavefront
constexpr int kJpeg420Threads = 6 * kJpeg420Mcus;   // a wavefront per block place, so a wavefront runs one of the two code paths
constexpr int kJpeg420RowDwords = 12;               // an MCU row: 16 pixels of 3 bytes
// an MCU in LDS: 16 rows, and one dword so that the lanes of a wavefront (consecutive MCUs, same row and column) hit different banks
constexpr int kJpeg420McuDwords = 16 * kJpeg420RowDwords + 1;
// k_jpeg_pack_rst's LDS image: kJpegPackDwords' terms, with up to 7 fill bits behind every block (a block ends at most one interval)
constexpr int kJpegPackDwordsRst = (31 + kJpegBlocks * (y2j::kBlockBitsMax + 7) + 31) / 32 + 1;

__device__ inline uint32_t jpeg_byte(const uint32_t *w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }   // (j is a constant after unrolling)

// grid (ceil(max MCUs / kJpeg420Mcus), frames)
__global__ __launch_bounds__(kJpeg420Threads) void k_jpeg_transform420(const uint8_t *__restrict__ table, const uint8_t *__restrict__ src_base,
                                                                       int16_t *__restrict__ coef)
{
    __shared__ float s_fd[2][64];
    __shared__ uint32_t s_px[kJpeg420Mcus * kJpeg420McuDwords];
    const JpegHeader *hd = reinterpret_cast<const JpegHeader *>(table);
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    const int tid = threadIdx.x, n_mcu = fr.n_blk / 6, mcu0 = (int)blockIdx.x * kJpeg420Mcus;
    if (mcu0 >= n_mcu) return;   // (the whole workgroup)
    if (tid < 128) s_fd[tid >> 6][tid & 63] = hd->t.fdtbl[tid >> 6][tid & 63];
    const int nm = min(kJpeg420Mcus, n_mcu - mcu0);
    const uint8_t *src = src_base + fr.src_off;
    // the MCUs' bytes, a dword of an MCU row per step (the source has any alignment and edge pixels repeat: byte loads)
    for (int j = tid; j < nm * 16 * kJpeg420RowDwords; j += kJpeg420Threads) {
        const int m = j / (16 * kJpeg420RowDwords), rem = j - m * (16 * kJpeg420RowDwords), r = rem / kJpeg420RowDwords, q = rem - r * kJpeg420RowDwords;
        const int mcu = mcu0 + m, my = mcu / fr.mcux, mx = mcu - my * fr.mcux;
        const uint8_t *row = src + (size_t)min(my * 16 + r, fr.h - 1) * fr.w * 3;
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int at = 4 * q + i, px = at / 3, ch = at - 3 * px;
            v |= (uint32_t)row[(size_t)min(mx * 16 + px, fr.w - 1) * 3 + ch] << (8 * i);
        }
        s_px[m * kJpeg420McuDwords + rem] = v;
    }
    __syncthreads();
    const int k = tid >> 6, m = tid & 63;   // block place (the same for a wavefront), MCU
    if (m >= nm) return;
    const int base = m * kJpeg420McuDwords;
    float d[64];
    if (k < 4) {   // a Y block: k_jpeg_transform's Y, operation for operation
        const int at = base + (k >> 1) * 8 * kJpeg420RowDwords + (k & 1) * 6;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint32_t w[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) w[i] = s_px[at + r * kJpeg420RowDwords + i];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float R = (float)jpeg_byte(w, 3 * c), G = (float)jpeg_byte(w, 3 * c + 1), B = (float)jpeg_byte(w, 3 * c + 2);
                d[r * 8 + c] = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(0.299f, R), __fmul_rn(0.587f, G)), __fmul_rn(0.114f, B)), 128.f);
            }
        }
    } else {       // Cb or Cr: the four values of a 2 x 2 as k_jpeg_transform computes them, then ((a + b) + (c + d)) * 0.25f
        const float c0 = k == 4 ? -0.16874f : 0.5f, c1 = k == 4 ? -0.33126f : -0.41869f, c2 = k == 4 ? 0.5f : -0.08131f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint32_t w[2][kJpeg420RowDwords];
#pragma unroll
            for (int i = 0; i < 2 * kJpeg420RowDwords; ++i) w[i / kJpeg420RowDwords][i % kJpeg420RowDwords] = s_px[base + 2 * r * kJpeg420RowDwords + i];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int at = 3 * (2 * c + (i & 1));
                    const float R = (float)jpeg_byte(w[i >> 1], at), G = (float)jpeg_byte(w[i >> 1], at + 1), B = (float)jpeg_byte(w[i >> 1], at + 2);
                    v[i] = __fadd_rn(__fadd_rn(__fmul_rn(c0, R), __fmul_rn(c1, G)), __fmul_rn(c2, B));
                }
                d[r * 8 + c] = __fmul_rn(__fadd_rn(__fadd_rn(v[0], v[1]), __fadd_rn(v[2], v[3])), 0.25f);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) jpeg_aan(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5], d[8 * r + 6], d[8 * r + 7]);
#pragma unroll
    for (int c = 0; c < 8; ++c) jpeg_aan(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
    uint32_t pk[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) pk[i] = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const float v = __fmul_rn(d[i], s_fd[k >= 4][i]);
        const int q = (int)(v < 0.f ? __fsub_rn(v, 0.5f) : __fadd_rn(v, 0.5f));
        const int z = y2j::kZigzag[i];
        pk[z >> 1] |= ((uint32_t)q & 0xffffu) << (16 * (z & 1));
    }
    uint4 *o = reinterpret_cast<uint4 *>(coef + ((size_t)fr.blk0 + (size_t)(mcu0 + m) * 6 + k) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = make_uint4(pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]);
}

// ---- the scan's operator

// A run of blocks as a function of the bit position p it starts at: seen ? ceil8(p + pre) + post : p + pre
template <typename T>
struct JpegRun {
    T pre, post;
    uint32_t seen;
    __device__ inline T at(T p) const { return seen ? ((p + pre + 7) & ~(T)7) + post : p + pre; }
};
// run a, then run b
template <typename T>
__device__ inline JpegRun<T> jpeg_run_then(const JpegRun<T> &a, const JpegRun<T> &b)
{
    if (!a.seen) return {a.pre + b.pre, b.post, b.seen};
    if (!b.seen) return {a.pre, a.post + b.pre, 1u};
    return {a.pre, ((a.post + b.pre + 7) & ~(T)7) + b.post, 1u};
}
// inclusive scan of one run per lane over a workgroup of N lanes (N a power of two), through the three arrays
template <int N, typename T>
__device__ inline JpegRun<T> jpeg_scan_runs(JpegRun<T> v, T *s_pre, T *s_post, uint32_t *s_seen, int tid)
{
    s_pre[tid] = v.pre; s_post[tid] = v.post; s_seen[tid] = v.seen;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < N; d <<= 1) {
        JpegRun<T> t = {0, 0, 0u};
        if (tid >= d) t = {s_pre[tid - d], s_post[tid - d], s_seen[tid - d]};
        __syncthreads();
        v = jpeg_run_then(t, v);
        s_pre[tid] = v.pre; s_post[tid] = v.post; s_seen[tid] = v.seen;
        __syncthreads();
    }
    return v;
}
__device__ inline JpegRun<uint32_t> jpeg_run_unpack(uint32_t pre, uint32_t post) { return {pre, post & 0x7fffffffu, post >> 31}; }

// what the mode makes of block b of a frame
struct JpegPlace {
    int pred_back;   // the DC predictor is the DC of block b - pred_back; 0: the predictor is zero
    bool luma, starts, ends;   // starts / ends an interval (the scan's end ends one)
    unsigned interval;
};
__device__ inline JpegPlace jpeg_place_of(const JpegFrame &fr, int b)
{
    const int bpm = y2j::mcu_blocks(fr.subsample), mcu = b / bpm, k = b - mcu * bpm, R = fr.restart ? fr.restart : fr.n_blk;
    const int in = mcu % R, back = y2j::dc_pred_back(fr.subsample, k);
    JpegPlace p;
    p.pred_back = in * bpm + k >= back ? back : 0;   // (zero where the component has no block in the interval yet)
    p.luma = y2j::block_is_luma(fr.subsample, k);
    p.starts = in == 0 && k == 0;
    p.ends = k == bpm - 1 && (in == R - 1 || b == fr.n_blk - 1);
    p.interval = (unsigned)(mcu / R);
    return p;
}

// grid (ceil(max n_blk / kJpegBlocks), frames)
template <bool kOpt>
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_lengths_rst(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                                  uint32_t *__restrict__ blk_off, uint32_t *__restrict__ blk_post,
                                                                  uint32_t *__restrict__ wg_sum, uint32_t *__restrict__ wg_post,
                                                                  const JpegOptFrame *__restrict__ opt)
{
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint32_t s_pre[kJpegBlocks], s_post[kJpegBlocks], s_seen[kJpegBlocks];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    jpeg_stage_codes<kOpt>(s_code, table, opt, blockIdx.y, tid, kJpegBlocks);
    __syncthreads();
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    JpegRun<uint32_t> own = {0u, 0u, 0u};
    if (b < fr.n_blk) {
        const size_t blk = (size_t)fr.blk0 + b;
        const JpegPlace pl = jpeg_place_of(fr, b);
        const uint32_t *dc = s_code + (pl.luma ? 0 : 2) * 256, *ac = dc + 256;
        JpegBlock c;
        c.load(coef, blk);
        const int pred = jpeg_dc_pred(coef, blk, pl.pred_back);
        const int cat = jpeg_category(c.at(0) - pred);
        uint32_t bits = (dc[cat] >> 16) + cat;
        int run = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int v = c.at(i);
            if (v == 0) {
                ++run;
            } else {
                const int k = jpeg_category(v);
                bits += (run >> 4) * (ac[0xF0] >> 16) + (ac[((run & 15) << 4) | k] >> 16) + k;
                run = 0;
            }
        }
        if (run) bits += ac[0] >> 16;
        own = {bits, 0u, pl.ends ? 1u : 0u};
    }
    const JpegRun<uint32_t> incl = jpeg_scan_runs<kJpegBlocks>(own, s_pre, s_post, s_seen, tid);
    if (b < fr.n_blk) {   // the run of the group's blocks before this one
        blk_off[(size_t)fr.blk0 + b] = tid ? s_pre[tid - 1] : 0u;
        blk_post[(size_t)fr.blk0 + b] = tid ? s_post[tid - 1] | s_seen[tid - 1] << 31 : 0u;
    }
    if (tid == kJpegBlocks - 1) {
        wg_sum[fr.wg0 + blockIdx.x] = incl.pre;
        wg_post[fr.wg0 + blockIdx.x] = incl.post | incl.seen << 31;
    }
}

// grid (frames): the groups' runs -> wg_base (where each group starts), the frame's totals; the end dwords zeroed as k_jpeg_scan_groups does
__global__ __launch_bounds__(kJpegScan) void k_jpeg_scan_groups_rst(const uint8_t *__restrict__ table, const uint32_t *__restrict__ wg_sum,
                                                                    const uint32_t *__restrict__ wg_post, unsigned long long *__restrict__ wg_base,
                                                                    uint8_t *__restrict__ us_base, JpegState *__restrict__ state)
{
    typedef unsigned long long u64;
    __shared__ u64 s_pre[kJpegScan], s_post[kJpegScan];
    __shared__ uint32_t s_seen[kJpegScan];
    const JpegFrame fr = jpeg_frame(table, blockIdx.x);
    const int tid = threadIdx.x;
    uint32_t *us = reinterpret_cast<uint32_t *>(us_base + fr.us_off);
    u64 running = 0;   // where the round's first group starts: the rounds before are a run applied to 0 already
    for (unsigned base = 0; base < fr.n_wg; base += kJpegScan) {
        const unsigned i = base + tid;
        JpegRun<u64> own = {0, 0, 0u};
        if (i < fr.n_wg) {
            const JpegRun<uint32_t> g = jpeg_run_unpack(wg_sum[fr.wg0 + i], wg_post[fr.wg0 + i]);
            own = {g.pre, g.post, g.seen};
        }
        const JpegRun<u64> incl = jpeg_scan_runs<kJpegScan>(own, s_pre, s_post, s_seen, tid);
        if (i < fr.n_wg) {
            JpegRun<u64> before = {0, 0, 0u};
            if (tid) before = {s_pre[tid - 1], s_post[tid - 1], s_seen[tid - 1]};
            const u64 lo = before.at(running), hi = incl.at(running);   // (hi > lo: a block has at least a DC code and an end-of-block)
            wg_base[fr.wg0 + i] = lo;
            us[lo >> 5] = 0u;
            us[(hi - 1) >> 5] = 0u;
        }
        const JpegRun<u64> all = {s_pre[kJpegScan - 1], s_post[kJpegScan - 1], s_seen[kJpegScan - 1]};
        running = all.at(running);
        __syncthreads();
    }
    if (tid == 0) {   // (the last block ends an interval: a multiple of 8)
        state[blockIdx.x].bits = running;
        state[blockIdx.x].ubytes = running >> 3;
    }
}

// grid (ceil(max n_blk / kJpegBlocks), frames)
template <bool kOpt>
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_pack_rst(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                               const uint32_t *__restrict__ blk_off, const uint32_t *__restrict__ blk_post,
                                                               const uint32_t *__restrict__ wg_sum, const uint32_t *__restrict__ wg_post,
                                                               const unsigned long long *__restrict__ wg_base, uint8_t *__restrict__ us_base,
                                                               uint32_t *__restrict__ rst_off, const JpegOptFrame *__restrict__ opt)
{
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint32_t s_bits[kJpegPackDwordsRst];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    jpeg_stage_codes<kOpt>(s_code, table, opt, blockIdx.y, tid, kJpegBlocks);
    const unsigned long long lo = wg_base[fr.wg0 + blockIdx.x], d0 = lo >> 5;
    // in the image bit 0 is the top bit of dword d0 of the stream: a multiple of 32 away, so rounding up to a byte is the same there
    const uint32_t first = (uint32_t)(lo - (d0 << 5));
    const uint32_t end = jpeg_run_unpack(wg_sum[fr.wg0 + blockIdx.x], wg_post[fr.wg0 + blockIdx.x]).at(first);
    const unsigned long long hi = (d0 << 5) + end;
    const int nd = (int)((end - 1) >> 5) + 1;
    for (int j = tid; j < nd + 1; j += kJpegBlocks) s_bits[j] = 0u;
    __syncthreads();
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    if (b < fr.n_blk) {
        const size_t blk = (size_t)fr.blk0 + b;
        const JpegPlace pl = jpeg_place_of(fr, b);
        const uint32_t *dc = s_code + (pl.luma ? 0 : 2) * 256, *ac = dc + 256;
        JpegBlock c;
        c.load(coef, blk);
        uint32_t pos = jpeg_run_unpack(blk_off[blk], blk_post[blk]).at(first);
        if (pl.starts) rst_off[fr.rst0 + pl.interval] = (uint32_t)(((d0 << 5) + pos) >> 3);   // (the entries refuse frames whose bound passes 2^31)
        const int pred = jpeg_dc_pred(coef, blk, pl.pred_back);
        const int diff = c.at(0) - pred, cat = jpeg_category(diff);
        jpeg_put(s_bits, pos, ((dc[cat] & 0xffffu) << cat) | jpeg_extra(diff, cat), (int)(dc[cat] >> 16) + cat);
        int run = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int v = c.at(i);
            if (v == 0) {
                ++run;
            } else {
                for (; run >= 16; run -= 16) jpeg_put(s_bits, pos, ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));
                const int k = jpeg_category(v);
                const uint32_t cw = ac[(run << 4) | k];
                jpeg_put(s_bits, pos, ((cw & 0xffffu) << k) | jpeg_extra(v, k), (int)(cw >> 16) + k);
                run = 0;
            }
        }
        if (run) jpeg_put(s_bits, pos, ac[0] & 0xffffu, (int)(ac[0] >> 16));
        const int fill = (int)((8 - (pos & 7)) & 7);
        if (pl.ends && fill) jpeg_put(s_bits, pos, (1u << fill) - 1u, fill);
    }
    __syncthreads();
    uint32_t *us = reinterpret_cast<uint32_t *>(us_base + fr.us_off);
    for (int j = tid; j < nd; j += kJpegBlocks) {
        const unsigned long long g = d0 + j;
        const uint32_t v = __builtin_bswap32(s_bits[j]);
        if ((g << 5) >= lo && ((g + 1) << 5) <= hi) us[g] = v;
        else atomicOr(&us[g], v);   // shared with a neighbour, or the frame's last, partial dword: zeroed by k_jpeg_scan_groups_rst
    }
}

// grid (ceil(frames / kJpegScan)): DRI and FF Dn between the intervals, which k_jpeg_scan_segs does not know of
__global__ __launch_bounds__(kJpegScan) void k_jpeg_sizes_rst(const uint8_t *__restrict__ table, JpegState *__restrict__ state,
                                                              unsigned long long *__restrict__ sizes, int nf)
{
    const int f = (int)(blockIdx.x * kJpegScan + threadIdx.x);
    if (f >= nf) return;
    const JpegFrame &fr = jpeg_frame(table, f);
    const unsigned long long size = state[f].size + (unsigned)(y2j::header_bytes(fr.restart) - y2j::kHeaderBytes) + 2ull * (fr.n_int - 1);
    state[f].size = size;
    sizes[f] = size;
}

// the interval that unstuffed byte x lies in, among intervals lo..hi (it lies in one of them): the last whose offset is <= x
__device__ inline unsigned jpeg_interval_of(const uint32_t *__restrict__ rst, unsigned lo, unsigned hi, unsigned long long x)
{
    while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (rst[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// grid (some, frames), as k_jpeg_count_ff
template <bool kOpt>
__global__ __launch_bounds__(kJpegSegThreads) void k_jpeg_emit_rst(const uint8_t *__restrict__ table, const uint8_t *__restrict__ us_base,
                                                                   const JpegState *__restrict__ state, const uint32_t *__restrict__ seg_base,
                                                                   const uint32_t *__restrict__ rst_off, uint8_t *__restrict__ out_base,
                                                                   const JpegOptFrame *__restrict__ opt)
{
    __shared__ uint32_t s_scan[kJpegSegThreads];
    __shared__ unsigned s_iv[2];
    const JpegHeader *hd = reinterpret_cast<const JpegHeader *>(table);
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    const JpegState st = state[blockIdx.y];
    uint8_t *out = out_base + st.out_off;
    const uint32_t *rst = rst_off + fr.rst0;
    const int tid = threadIdx.x, head = kOpt ? (int)opt[blockIdx.y].head_len : y2j::header_bytes(fr.restart);
    if (blockIdx.x == 0) {
        for (int i = tid; i < head; i += kJpegSegThreads)
            if ((unsigned long long)i < fr.cap)
                out[i] = kOpt ? opt[blockIdx.y].header[i] : y2j::header_byte(hd->t.header, i, fr.w, fr.h, fr.subsample, fr.restart);
        if (tid < 2 && st.size - 2 + tid < fr.cap) out[st.size - 2 + tid] = tid ? 0xD9 : 0xFF;   // EOI
    }
    const unsigned nseg = (unsigned)((st.ubytes + kJpegSegBytes - 1) / kJpegSegBytes);
    for (unsigned seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const unsigned long long seg_at = (unsigned long long)seg * kJpegSegBytes;
        // the segment's base: the intervals its first and its last byte lie in
        if (tid < 2) {
            const unsigned long long last = seg_at + kJpegSegBytes < st.ubytes ? seg_at + kJpegSegBytes - 1 : st.ubytes - 1;
            s_iv[tid] = jpeg_interval_of(rst, 0u, fr.n_int - 1, tid ? last : seg_at);
        }
        uint32_t w[4];
        const unsigned long long at = seg_at + tid * 16;
        const int ff = jpeg_seg_load(us_base + fr.us_off, st.ubytes, at, w);
        const uint32_t incl = jpeg_scan_incl<kJpegSegThreads>((uint32_t)ff, s_scan, tid);   // (its barriers publish s_iv)
        if (at < st.ubytes) {
            const unsigned iv_hi = s_iv[1];
            unsigned iv = jpeg_interval_of(rst, s_iv[0], iv_hi, at);
            unsigned long long next = iv < iv_hi ? rst[iv + 1] : ~0ull;   // where the next interval starts
            unsigned long long o = (unsigned long long)head + at + seg_base[fr.seg0 + seg] + (incl - (uint32_t)ff) + 2ull * iv;
            const bool at_start = iv && rst[iv] == at;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint8_t v = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
                if (at + i < st.ubytes) {
                    bool marker = i == 0 && at_start;
                    if (at + i == next) {   // (an interval has at least one byte: one step)
                        ++iv;
                        o += 2;
                        next = iv < iv_hi ? rst[iv + 1] : ~0ull;
                        marker = true;
                    }
                    if (marker) {   // FF Dn of the interval before, in front of this interval's first byte; never stuffed
                        if (o - 2 < fr.cap) out[o - 2] = 0xFF;
                        if (o - 1 < fr.cap) out[o - 1] = (uint8_t)(0xD0 + ((iv - 1) & 7u));
                    }
                    if (o < fr.cap) out[o] = v;
                    ++o;
                    if (v == 255) {
                        if (o < fr.cap) out[o] = 0;
                        ++o;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ================================================================================================ optimize (jpeg_opt.hpp)
//
// optimize = 1 puts three launches between stage A and stage B and runs the <true> forms of the kernels that read code words or the
// header; the transforms, k_jpeg_count_ff, the scans and k_jpeg_place run as they are.
//   k_jpeg_hist_clear      the chunk's counts to zero (a kernel, so that the sequence can be captured into a graph)
//   k_jpeg_hist            a workgroup per kJpegBlocks blocks, a lane per block (stage B's split and its jpeg_place_of / jpeg_dc_pred):
//                          the block's symbols counted into the lane's WAVEFRONT's copy of the 536 bins in LDS - end-of-block, sixteen
//                          zeros and the small (run, size) symbols are hit by nearly every lane, and one copy would serialise all of
//                          them - then the copies are added up and the non-zero sums go to hist[frame] with integer atomics
//   k_jpeg_opt_tables      a workgroup per frame, a wavefront per table: all lanes rank-sort the (count, symbol) keys (distinct, so
//                          the ranks are the host's order), lane 0 runs the tree, the limit and the per-length firsts of jpeg_opt.hpp
//                          with every variably indexed array in LDS; after a barrier all four wavefronts add up both costs, and
//                          after the next every lane knows the decision: the frame's code words (each lane its symbols' rank within
//                          their length) or the standard ones go to JpegOptFrame, the DHT payload is put together in LDS and the
//                          header's bytes are written by all lanes
//   k_jpeg_sizes_opt       the sizes k_jpeg_scan_segs (and k_jpeg_sizes_rst) left, with the frame's header length in place of the
//                          standard one
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.10.3.

constexpr int kJpegHistWaves = kJpegBlocks / 64;
constexpr int kJpegOptThreads = 4 * 64;   // a wavefront per table

// grid (ceil(n / kJpegScan)), n = frames * kOptHistBins
__global__ __launch_bounds__(kJpegScan) void k_jpeg_hist_clear(uint32_t *__restrict__ hist, int n)
{
    const int i = (int)(blockIdx.x * kJpegScan + threadIdx.x);
    if (i < n) hist[i] = 0u;
}

// grid (ceil(max n_blk / kJpegBlocks), frames)
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_hist(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                           uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_h[kJpegHistWaves][y2j::kOptHistBins];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    for (int i = tid; i < kJpegHistWaves * y2j::kOptHistBins; i += kJpegBlocks) (&s_h[0][0])[i] = 0u;
    __syncthreads();
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    if (b < fr.n_blk) {
        const size_t blk = (size_t)fr.blk0 + b;
        const JpegPlace pl = jpeg_place_of(fr, b);
        uint32_t *dc = s_h[tid >> 6] + y2j::opt_hist_at(pl.luma ? y2j::kDcLuma : y2j::kDcChroma);
        uint32_t *ac = s_h[tid >> 6] + y2j::opt_hist_at(pl.luma ? y2j::kAcLuma : y2j::kAcChroma);
        JpegBlock c;
        c.load(coef, blk);
        atomicAdd(&dc[jpeg_category(c.at(0) - jpeg_dc_pred(coef, blk, pl.pred_back))], 1u);
        int run = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int v = c.at(i);
            if (v == 0) {
                ++run;
            } else {
                if (run >= 16) atomicAdd(&ac[0xF0], (uint32_t)(run >> 4));
                atomicAdd(&ac[((run & 15) << 4) | jpeg_category(v)], 1u);
                run = 0;
            }
        }
        if (run) atomicAdd(&ac[0], 1u);
    }
    __syncthreads();
    for (int i = tid; i < y2j::kOptHistBins; i += kJpegBlocks) {
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kJpegHistWaves; ++k) sum += s_h[k][i];
        if (sum) atomicAdd(&hist[(size_t)blockIdx.y * y2j::kOptHistBins + i], sum);
    }
}

// grid (frames)
__global__ __launch_bounds__(kJpegOptThreads) void k_jpeg_opt_tables(const uint8_t *__restrict__ table, const uint32_t *__restrict__ hist,
                                                                     JpegOptFrame *__restrict__ opt)
{
    __shared__ y2j::OptScratch s_w[4];
    __shared__ uint32_t s_hist[y2j::kOptHistBins];
    __shared__ uint8_t s_dht[y2j::kDhtStdPayload];
    __shared__ uint32_t s_n[4], s_used[4];
    __shared__ unsigned long long s_total[4], s_cost[2];
    const JpegHeader *hd = reinterpret_cast<const JpegHeader *>(table);
    const JpegFrame fr = jpeg_frame(table, blockIdx.x);
    const int tid = threadIdx.x, t = tid >> 6, lane = tid & 63;   // t: the wavefront's table, kDcLuma .. kAcChroma
    y2j::OptScratch &w = s_w[t];
    const int nsym = y2j::opt_syms(t);
    for (int i = tid; i < y2j::kOptHistBins; i += kJpegOptThreads) s_hist[i] = hist[(size_t)blockIdx.x * y2j::kOptHistBins + i];
    if (tid < 4) { s_n[tid] = 0u; s_used[tid] = 0u; s_total[tid] = 0ull; }
    if (tid < 2) s_cost[tid] = 0ull;
    for (int q = lane; q <= y2j::kOptReserved; q += 64) w.len[q] = 0;
    __syncthreads();
    const uint32_t *ht = s_hist + y2j::opt_hist_at(t);
    {
        unsigned long long total = 0;
        uint32_t used = 0;
        for (int q = lane; q < nsym; q += 64) { total += ht[q]; used += ht[q] != 0u; }
        atomicAdd(&s_total[t], total);
        atomicAdd(&s_n[t], used);
    }
    __syncthreads();
    const bool built = s_total[t] < y2j::kOptCountLimit;   // (a count fits its key)
    const int n = 1 + (int)s_n[t];                         // the keys: the symbols in use and the reserved one, the smallest
    if (built) {
        for (int q = lane; q < nsym; q += 64) {
            if (!ht[q]) continue;
            const uint32_t key = (ht[q] << 9) | (uint32_t)q;
            int rank = 1;
            for (int r = 0; r < nsym; ++r) rank += ht[r] != 0u && ((ht[r] << 9) | (uint32_t)r) < key;
            w.h.key[rank] = key;
        }
        if (lane == 0) w.h.key[0] = (uint32_t)y2j::kOptReserved;
    }
    __syncthreads();
    if (built && lane == 0) {
        if (n >= 2) y2j::opt_lengths(w, n, y2j::opt_maxlen(t));
        s_used[t] = (uint32_t)y2j::opt_canon_prepare(w, nsym);
    }
    __syncthreads();
    {   // both costs: the code bits of the frame's symbols under either table set
        unsigned long long own = 0, standard = 0;
        for (int q = lane; q < nsym; q += 64) {
            own += (unsigned long long)ht[q] * w.len[q];
            standard += (unsigned long long)ht[q] * (hd->t.code[t][q] >> 16);
        }
        atomicAdd(&s_cost[0], own);
        atomicAdd(&s_cost[1], standard);
    }
    __syncthreads();
    bool use = true;
    int payload = 0, off = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        use = use && s_total[k] < y2j::kOptCountLimit;
        if (k < t) off += 17 + (int)s_used[k];
        payload += 17 + (int)s_used[k];
    }
    use = use && payload <= y2j::kDhtStdPayload;   // (more symbols than T.81 has: not from 8-bit pixels)
    use = use && s_cost[0] + 8ull * (unsigned)payload < s_cost[1] + 8ull * y2j::kDhtStdPayload;   // (the same for every lane)
    JpegOptFrame &of = opt[blockIdx.x];
    if (use) {
        if (lane == 0) s_dht[off] = (uint8_t)y2j::opt_dht_id(t);
        if (lane >= 1 && lane <= 16) s_dht[off + lane] = (uint8_t)w.h.count[lane];
    }
    for (int q = lane; q < 256; q += 64) {
        uint32_t code = use ? 0u : hd->t.code[t][q];
        if (use && q < nsym && w.len[q]) {
            int place;
            code = y2j::opt_canon_symbol(w, q, &place);
            s_dht[off + 17 + place] = (uint8_t)q;
        }
        of.code[t][q] = code;
    }
    __syncthreads();
    const int head = use ? y2j::opt_header_len(payload, fr.restart) : y2j::header_bytes(fr.restart);
    for (int i = tid; i < head; i += kJpegOptThreads)
        of.header[i] = use ? y2j::opt_header_byte(hd->t.header, i, fr.w, fr.h, fr.subsample, fr.restart, s_dht, payload)
                           : y2j::header_byte(hd->t.header, i, fr.w, fr.h, fr.subsample, fr.restart);
    if (tid == 0) {
        of.head_len = (uint32_t)head;
        of.used = use ? 1u : 0u;
    }
}

// grid (ceil(frames / kJpegScan))
__global__ __launch_bounds__(kJpegScan) void k_jpeg_sizes_opt(const uint8_t *__restrict__ table, const JpegOptFrame *__restrict__ opt,
                                                              JpegState *__restrict__ state, unsigned long long *__restrict__ sizes, int nf)
{
    const int f = (int)(blockIdx.x * kJpegScan + threadIdx.x);
    if (f >= nf) return;
    const unsigned long long size = state[f].size - (unsigned)y2j::header_bytes(jpeg_frame(table, f).restart) + opt[f].head_len;
    state[f].size = size;
    sizes[f] = size;
}

}  // namespace y2

