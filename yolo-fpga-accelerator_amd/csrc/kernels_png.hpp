// kernels_png.hpp -- bytes in device memory -> zlib streams of dynamic-Huffman deflate blocks without LZ matches, by the definition of
// png_huff.hpp (the deflate stage of the library's PNG files): histograms, Huffman codes, bit offsets, bit packing, Adler-32 and
// framing, batched over the streams of a chunk.  Six launches, nothing read back between them (yolo2_png.hip lays the work area out):
//   k_png_hist    grid (blocks, streams)  a 257-bin histogram per deflate block, privatised per wavefront in LDS, one merge; the
//                                         block's Adler-32 sums on the way
//   k_png_codes   grid (all blocks / 4)   one wavefront per block: rank sort by all lanes, then the tree, the length limit, the codes
//                                         and the header bits by lane 0 through png_huff.hpp (the text the host runs), the table out
//                                         by all lanes as [block][257] code | len << 16
//   k_png_scan    one lane per stream     bit offsets of the blocks (a stored block's padding depends on where it starts), Adler-32
//                                         combine; clears the words that two blocks share
//   k_png_pack    grid (blocks, streams)  the block staged in LDS, a lane per kPngSeg bytes: bit counts, a workgroup scan, then codes
//                                         into a 64-bit LSB-first accumulator; whole-word stores inside a lane's run, its first word
//                                         ORed in after a barrier, words shared between blocks by atomic OR
//   k_png_emit    grid (tiles, streams)   deflate data -> the caller's buffer (any alignment) through LDS
//   k_png_finish  one lane per stream     zlib header, Adler-32, the size
// Vector stores only; no scratch (every variably indexed array is in LDS).
#pragma once
#include <hip/hip_runtime.h>

#include "png_huff.hpp"

namespace y2 {

constexpr int kPngThreads = 256, kPngWaves = kPngThreads / 64;
constexpr int kPngSeg = y2p::kBlock / kPngThreads; // input bytes per pack lane (128)
constexpr int kPngTile = kPngThreads * 16;         // deflate bytes per emit workgroup
static_assert(kPngSeg % 4 == 0 && kPngSeg * kPngThreads == (int)y2p::kBlock, "a lane per segment");

struct PngStream {           // one stream of the chunk
    size_t src_off;          // the input bytes in src_base
    size_t ds_off;           // work: the deflate data, 256-byte aligned
    size_t out_off;          // the stream in out_base
    size_t n;                // bytes to deflate
    uint32_t blk0, n_blk;    // its deflate blocks in the chunk's per-block arrays
};
struct PngBlock {
    unsigned long long bit0;   // where the block starts in the stream's deflate data
    uint32_t dyn_bits, blen, flags, pa, pb, stream;   // flags: 1 stored, 2 last block; pa, pb: Adler-32 sums of the block
};
struct PngState {
    unsigned long long total_bits, size;
    uint32_t adler, pad;
};

__device__ __forceinline__ uint32_t png_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// a row (or block) of n bytes at p, fetched as aligned dwords: dword d of the window holds bytes 4 d - a .. 4 d - a + 3 of it
struct PngWindow {
    const uint32_t *q;
    uint32_t a, nd;
    __device__ PngWindow(const uint8_t *p, uint32_t n) : q(reinterpret_cast<const uint32_t *>(p - ((uintptr_t)p & 3))), a((uint32_t)((uintptr_t)p & 3)), nd((a + n + 3) >> 2) {}
};

// ---------------------------------------------------------------------------------------------------------------- histogram
__global__ __launch_bounds__(kPngThreads) void k_png_hist(const PngStream *__restrict__ streams, const uint8_t *__restrict__ src_base,
                                                          const uint8_t *__restrict__ work, uint32_t *__restrict__ hist, PngBlock *__restrict__ blocks)
{
    __shared__ uint32_t s_h[kPngWaves][y2p::kLitSyms];
    __shared__ uint32_t s_sum[kPngWaves][2];
    const PngStream fr = streams[blockIdx.y];
    if (blockIdx.x >= fr.n_blk) return;
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint32_t len = y2p::block_len(fr.n, blockIdx.x);
    const PngWindow win((src_base + fr.src_off) + (size_t)blockIdx.x * y2p::kBlock, len);
    for (int s = tid; s < kPngWaves * y2p::kLitSyms; s += kPngThreads) (&s_h[0][0])[s] = 0;
    __syncthreads();
    uint32_t pa = 0, pb = 0;   // (a lane sees at most 132 bytes: pb < 132 * 255 * 32768 < 2^32)
    for (uint32_t d = tid; len && d < win.nd; d += kPngThreads) {
        const uint32_t v4 = win.q[d];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t o = 4 * d + k - win.a;   // (wraps below the window: o >= len)
            if (o < len) {
                const uint32_t v = (v4 >> (8 * k)) & 255u;
                atomicAdd(&s_h[wave][v], 1u);
                pa += v;
                pb += (len - o) * v;
            }
        }
    }
    pa = png_wave_sum(pa);
    pb = png_wave_sum(pb % y2p::kAdlerMod);
    if ((tid & 63) == 0) { s_sum[wave][0] = pa; s_sum[wave][1] = pb; }
    __syncthreads();
    const size_t g = fr.blk0 + blockIdx.x;
    for (int s = tid; s < y2p::kLitSyms; s += kPngThreads) {
        uint32_t c = 0;
#pragma unroll
        for (int v = 0; v < kPngWaves; ++v) c += s_h[v][s];
        hist[g * y2p::kLitSyms + s] = s == y2p::kEob ? 1u : c;
    }
    if (tid == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int v = 0; v < kPngWaves; ++v) { a += s_sum[v][0]; b += s_sum[v][1]; }
        PngBlock bl;
        bl.bit0 = 0; bl.dyn_bits = 0; bl.blen = len;
        bl.flags = blockIdx.x + 1 == fr.n_blk ? 2u : 0u;
        bl.pa = a % y2p::kAdlerMod; bl.pb = b % y2p::kAdlerMod; bl.stream = blockIdx.y;
        blocks[g] = bl;
    }
}

// ---------------------------------------------------------------------------------------------------------------- codes
__global__ __launch_bounds__(kPngThreads) void k_png_codes(const uint32_t *__restrict__ hist, uint32_t *__restrict__ codes, uint8_t *__restrict__ hdr,
                                                           PngBlock *__restrict__ blocks, uint32_t total_blocks)
{
    __shared__ y2p::HuffScratch s_w[kPngWaves];
    __shared__ y2p::BlockHeader s_hd[kPngWaves];
    __shared__ uint32_t s_hist[kPngWaves][y2p::kLitSyms], s_code[kPngWaves][y2p::kLitSyms];
    __shared__ uint8_t s_len[kPngWaves][y2p::kLitSyms + 3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t g = blockIdx.x * kPngWaves + wave;
    const bool active = g < total_blocks;
    if (active)
        for (int s = lane; s < y2p::kLitSyms; s += 64) s_hist[wave][s] = hist[(size_t)g * y2p::kLitSyms + s];
    __syncthreads();
    int n_used = 0;
    if (active) {   // rank sort: a key's place is the number of keys below it (keys are distinct)
        for (int s0 = 0; s0 < y2p::kLitSyms; s0 += 64) {
            const int s = s0 + lane;
            const uint32_t h = s < y2p::kLitSyms ? s_hist[wave][s] : 0u, key = (h << 9) | (uint32_t)s;
            if (h) {
                int rank = 0;
                for (int t = 0; t < y2p::kLitSyms; ++t) {
                    const uint32_t ht = s_hist[wave][t];
                    rank += (ht && ((ht << 9) | (uint32_t)t) < key) ? 1 : 0;
                }
                s_w[wave].key[rank] = key;
            }
            n_used += __popcll(__ballot(h != 0));
        }
    }
    __syncthreads();
    if (active && lane == 0) {   // the host's text: tree, length limit, code-length code, sizes, codes, header
        uint32_t flags = blocks[g].flags;
        y2p::code_lengths(s_hist[wave], y2p::kLitSyms, y2p::kLitMaxLen, s_w[wave], s_len[wave], true, n_used);
        y2p::plan_header(s_hist[wave], s_len[wave], blocks[g].blen, s_w[wave], &s_hd[wave]);
        if (s_hd[wave].stored) {
            for (int s = 0; s < 256; ++s) s_code[wave][s] = (uint32_t)s | (8u << 16);   // bytes as they are; no end-of-block code
            s_code[wave][y2p::kEob] = 0;
            flags |= 1u;
        } else {
            y2p::canonical_codes(s_len[wave], y2p::kLitSyms, s_w[wave], s_code[wave]);
            y2p::ByteBits bits(hdr + (size_t)g * y2p::kHdrBytes);
            y2p::write_header(bits, (flags & 2u) != 0, s_len[wave], s_hd[wave]);
            bits.align();
        }
        blocks[g].dyn_bits = s_hd[wave].dyn_bits;
        blocks[g].flags = flags;
    }
    __syncthreads();
    if (active)
        for (int s = lane; s < y2p::kLitSyms; s += 64) codes[(size_t)g * y2p::kLitSyms + s] = s_code[wave][s];
}

// ---------------------------------------------------------------------------------------------------------------- offsets
__global__ __launch_bounds__(64) void k_png_scan(const PngStream *__restrict__ streams, int n_streams, PngBlock *__restrict__ blocks,
                                                 uint8_t *__restrict__ work, PngState *__restrict__ state)
{
    const int f = (int)(blockIdx.x * 64 + threadIdx.x);
    if (f >= n_streams) return;
    const PngStream fr = streams[f];
    unsigned long long *ds = reinterpret_cast<unsigned long long *>(work + fr.ds_off);
    unsigned long long at = 0;
    uint32_t a = 1, b = 0;
    for (uint32_t i = 0; i < fr.n_blk; ++i) {
        PngBlock &bl = blocks[fr.blk0 + i];
        bl.bit0 = at;
        if (at & 63) ds[at >> 6] = 0;   // shared with the block before: both sides OR into it
        at += y2p::block_bits(at, (bl.flags & 1u) != 0, bl.dyn_bits, bl.blen);
        y2p::adler_append(a, b, bl.pa, bl.pb, bl.blen);
    }
    if (at & 63) ds[at >> 6] = 0;
    PngState st;
    st.total_bits = at; st.size = 0; st.adler = (b << 16) | a; st.pad = 0;
    state[f] = st;
}

// ---------------------------------------------------------------------------------------------------------------- pack
// LDS index of dword d of the staged block: a pad dword after every 32, so that lanes kPngSeg bytes apart read different banks
__device__ __forceinline__ uint32_t png_pad(uint32_t d) { return d + (d >> 5); }

__global__ __launch_bounds__(kPngThreads) void k_png_pack(const PngStream *__restrict__ streams, const uint8_t *__restrict__ src_base,
                                                          uint8_t *__restrict__ work, const uint32_t *__restrict__ codes, const uint8_t *__restrict__ hdr,
                                                          const PngBlock *__restrict__ blocks)
{
    constexpr uint32_t kStageDwords = y2p::kBlock / 4 + 1;
    __shared__ uint32_t s_in[kStageDwords + kStageDwords / 32 + 1];
    __shared__ uint32_t s_code[y2p::kLitSyms];
    __shared__ uint32_t s_wave[kPngWaves];
    const PngStream fr = streams[blockIdx.y];
    if (blockIdx.x >= fr.n_blk) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t g = fr.blk0 + blockIdx.x;
    const PngBlock bl = blocks[g];
    const uint32_t len = bl.blen;
    const bool stored = (bl.flags & 1u) != 0;
    const PngWindow win((src_base + fr.src_off) + (size_t)blockIdx.x * y2p::kBlock, len);
    for (uint32_t d = tid; len && d < win.nd; d += kPngThreads) s_in[png_pad(d)] = win.q[d];
    for (int s = tid; s < y2p::kLitSyms; s += kPngThreads) s_code[s] = codes[g * y2p::kLitSyms + s];
    __syncthreads();

    // this lane's run: [the header] its segment's codes [the end-of-block code]
    const uint32_t n_seg = (len + kPngSeg - 1) / kPngSeg, last_lane = n_seg ? n_seg - 1 : 0;
    const uint32_t o0 = min(len, (uint32_t)tid * kPngSeg) + win.a, o1 = min(len, (uint32_t)(tid + 1) * kPngSeg) + win.a;   // window bytes
    const uint32_t pad = (uint32_t)((0 - (bl.bit0 + 3)) & 7);
    uint32_t bits = 0;
    for (uint32_t d = o0 >> 2; o0 < o1 && d <= (o1 - 1) >> 2; ++d) {
        const uint32_t v4 = s_in[png_pad(d)];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t o = 4 * d + k;
            if (o >= o0 && o < o1) bits += s_code[(v4 >> (8 * k)) & 255u] >> 16;
        }
    }
    if ((uint32_t)tid == last_lane) bits += s_code[y2p::kEob] >> 16;
    uint32_t incl = bits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int v = 0; v < kPngWaves; ++v) {
        if (v < wave) before += s_wave[v];
        all += s_wave[v];
    }
    const uint32_t head_bits = stored ? 3 + pad + 32 : bl.dyn_bits - all;   // (dyn_bits is the header and every code of the block)
    const unsigned long long end = bl.bit0 + head_bits + all;
    const unsigned long long p0 = tid == 0 ? bl.bit0 : bl.bit0 + head_bits + before + incl - bits;
    const unsigned long long edge0 = (bl.bit0 & 63) ? bl.bit0 >> 6 : ~0ull, edge1 = (end & 63) ? end >> 6 : ~0ull;

    unsigned long long *ds = reinterpret_cast<unsigned long long *>(work + fr.ds_off);
    unsigned long long acc = 0, wi = p0 >> 6, head_w = 0, head_v = 0;
    uint32_t fill = (uint32_t)(p0 & 63);
    bool first = fill != 0, have_head = false;   // first: the word the run starts in belongs to the lane before
    auto flush = [&](unsigned long long v) {
        if (wi == edge0 || wi == edge1) atomicOr(&ds[wi], v);   // shared with another workgroup; k_png_scan cleared it
        else if (first) { head_w = wi; head_v = v; have_head = true; }
        else ds[wi] = v;
        first = false;
        ++wi;
    };
    auto put = [&](uint32_t v, uint32_t n) {   // n <= 32, v below 2^n
        acc |= (unsigned long long)v << fill;
        if (fill + n >= 64) {
            flush(acc);
            acc = fill + n > 64 ? (unsigned long long)v >> (64 - fill) : 0ull;
            fill = fill + n - 64;
        } else {
            fill += n;
        }
    };
    if (tid == 0) {
        if (stored) {
            put((bl.flags >> 1) & 1u, 3);
            if (pad) put(0u, pad);
            put(len | ((~len & 0xffffu) << 16), 32);
        } else {
            const uint32_t *hw = reinterpret_cast<const uint32_t *>(hdr + g * y2p::kHdrBytes);
            uint32_t k = 0;
            const uint32_t take = min(head_bits, (uint32_t)y2p::kHdrBitsMax);   // (never past the slot, whatever the table says)
            for (; 32 * (k + 1) <= take; ++k) put(hw[k], 32);
            const uint32_t rest = take - 32 * k;
            if (rest) put(hw[k] & ((1u << rest) - 1u), rest);
        }
    }
    for (uint32_t d = o0 >> 2; o0 < o1 && d <= (o1 - 1) >> 2; ++d) {
        const uint32_t v4 = s_in[png_pad(d)];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t o = 4 * d + k;
            if (o >= o0 && o < o1) {
                const uint32_t c = s_code[(v4 >> (8 * k)) & 255u];
                put(c & 0xffffu, c >> 16);
            }
        }
    }
    if ((uint32_t)tid == last_lane && !stored) put(s_code[y2p::kEob] & 0xffffu, s_code[y2p::kEob] >> 16);
    if (fill) flush(acc);
    __threadfence();
    __syncthreads();   // every lane's last word is stored: now the neighbours' first bits go in
    if (have_head) atomicOr(&ds[head_w], head_v);
}

// ---------------------------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(kPngThreads) void k_png_emit(const PngStream *__restrict__ streams, const uint8_t *__restrict__ work,
                                                          const PngState *__restrict__ state, uint8_t *__restrict__ out_base)
{
    __shared__ uint4 s_tile[kPngThreads];
    const PngStream fr = streams[blockIdx.y];
    const size_t nd = (size_t)((state[blockIdx.y].total_bits + 7) >> 3), t0 = (size_t)blockIdx.x * kPngTile;
    if (t0 >= nd) return;
    const int tid = threadIdx.x;
    const size_t t1 = min(nd, t0 + kPngTile);
    s_tile[tid] = reinterpret_cast<const uint4 *>(work + fr.ds_off + t0)[tid];   // (the work area is padded to whole tiles)
    __syncthreads();
    // the tile to its place behind 78 01: bytes up to the first dword boundary, dwords, bytes
    uint8_t *dst = out_base + fr.out_off + 2 + t0;
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_tile);
    const uint32_t tb = (uint32_t)(t1 - t0), head = min(tb, (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3)), body = (tb - head) >> 2, tail = (tb - head) & 3;
    if ((uint32_t)tid < head) dst[tid] = sb[tid];
    for (uint32_t j = tid; j < body; j += kPngThreads) {
        const uint32_t o = head + 4 * j;
        *reinterpret_cast<uint32_t *>(dst + o) = sb[o] | ((uint32_t)sb[o + 1] << 8) | ((uint32_t)sb[o + 2] << 16) | ((uint32_t)sb[o + 3] << 24);
    }
    if ((uint32_t)tid < tail) dst[head + 4 * body + tid] = sb[head + 4 * body + tid];
}

// ---------------------------------------------------------------------------------------------------------------- framing
__global__ __launch_bounds__(64) void k_png_finish(const PngStream *__restrict__ streams, int n_streams, const PngState *__restrict__ state,
                                                   uint8_t *__restrict__ out_base, unsigned long long *__restrict__ sizes)
{
    const int f = (int)(blockIdx.x * 64 + threadIdx.x);
    if (f >= n_streams) return;
    const PngStream fr = streams[f];
    const PngState st = state[f];
    const size_t nd = (size_t)((st.total_bits + 7) >> 3);
    uint8_t *o = out_base + fr.out_off;
    o[0] = 0x78; o[1] = 0x01;
    y2p::put_be32(o + 2 + nd, st.adler);
    sizes[f] = 2 + nd + 4;
}

}  // namespace y2
