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
// The tables (fdtbl, code words, header) come from csrc/jpeg_tables.hpp on the host and lead the chunk's table.
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
    int n_blk;                    // 3 * MCUs
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

__device__ inline void jpeg_stage_codes(uint32_t *s_code, const uint8_t *table, int tid, int threads)
{
    const uint32_t *code = &reinterpret_cast<const JpegHeader *>(table)->t.code[0][0];
    for (int i = tid; i < 4 * 256; i += threads) s_code[i] = code[i];
}

// grid (ceil(max n_blk / kJpegBlocks), frames)
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_lengths(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                              uint32_t *__restrict__ blk_off, uint32_t *__restrict__ wg_sum)
{
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint32_t s_scan[kJpegBlocks];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    jpeg_stage_codes(s_code, table, tid, kJpegBlocks);
    __syncthreads();
    const int b = (int)blockIdx.x * kJpegBlocks + tid;
    uint32_t bits = 0;
    if (b < fr.n_blk) {
        const size_t blk = (size_t)fr.blk0 + b;
        const uint32_t *dc = s_code + (b % 3 ? 2 : 0) * 256, *ac = dc + 256;
        JpegBlock c;
        c.load(coef, blk);
        const int pred = b >= 3 ? (int)coef[(blk - 3) * 64] : 0;
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
__global__ __launch_bounds__(kJpegBlocks) void k_jpeg_pack(const uint8_t *__restrict__ table, const int16_t *__restrict__ coef,
                                                           const uint32_t *__restrict__ blk_off, const uint32_t *__restrict__ wg_sum,
                                                           const unsigned long long *__restrict__ wg_base, uint8_t *__restrict__ us_base)
{
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint32_t s_bits[kJpegPackDwords];
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    if (blockIdx.x >= fr.n_wg) return;   // (the whole workgroup)
    const int tid = threadIdx.x;
    jpeg_stage_codes(s_code, table, tid, kJpegBlocks);
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
        const int pred = b >= 3 ? (int)coef[(blk - 3) * 64] : 0;
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
__global__ __launch_bounds__(kJpegSegThreads) void k_jpeg_emit(const uint8_t *__restrict__ table, const uint8_t *__restrict__ us_base,
                                                               const JpegState *__restrict__ state, const uint32_t *__restrict__ seg_base,
                                                               uint8_t *__restrict__ out_base)
{
    __shared__ uint32_t s_scan[kJpegSegThreads];
    const JpegHeader *hd = reinterpret_cast<const JpegHeader *>(table);
    const JpegFrame fr = jpeg_frame(table, blockIdx.y);
    const JpegState st = state[blockIdx.y];
    uint8_t *out = out_base + st.out_off;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        for (int i = tid; i < y2j::kHeaderBytes; i += kJpegSegThreads) {
            uint8_t v = hd->t.header[i];
            if (i == y2j::kHeaderHeightAt) v = (uint8_t)(fr.h >> 8);
            if (i == y2j::kHeaderHeightAt + 1) v = (uint8_t)fr.h;
            if (i == y2j::kHeaderWidthAt) v = (uint8_t)(fr.w >> 8);
            if (i == y2j::kHeaderWidthAt + 1) v = (uint8_t)fr.w;
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
        unsigned long long o = (unsigned long long)y2j::kHeaderBytes + at + seg_base[fr.seg0 + seg] + (incl - (uint32_t)ff);
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

}  // namespace y2
