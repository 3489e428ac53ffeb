// png_huff.hpp -- the annotated frame as a PNG file, the library's own definition (include/yolo2_hip.h, "annotated frames as PNG"):
// a valid 8-bit RGB PNG whose rows are filtered by the rule of the reference's writer and whose IDAT is a zlib stream of
// dynamic-Huffman deflate blocks WITHOUT LZ matches.  Plain C++, no HIP includes: the kernels (kernels_png.hpp), the host writer
// (host/y2_png.cpp) and the CPU tests compile this one statement of the format, so the GPU's and the host's streams are equal byte
// for byte.  Byte identity with stb_image_write's PNG is NOT the definition: its zlib is a serial hash-chain LZ77 with fixed codes.
//
//   row filter   the five PNG filters with bpp = 3, each scored by the sum of abs((int8_t)byte) over the row; the first filter, in
//                order 0..4, with the strictly smallest score is taken; bytes outside the image are zero, which is what the "no row
//                above" forms of the first row come to.  (stb_image_write v1.09, stbi_write_png_to_mem with
//                stbi_write_force_png_filter < 0, and stbiw__encode_png_line: the rule, restated.)
//   deflate      blocks of kBlock input bytes, BTYPE = 2, BFINAL on the last.  Literal/length alphabet 0..255 and 256 (HLIT = 0), one
//                distance code of zero bits (HDIST = 0, RFC 1951 3.2.7).  Code lengths: Huffman over the symbols sorted by (count,
//                symbol), ties between a leaf and an inner node go to the leaf, limited to 15 bits (7 for the code-length code) by
//                moving codes between lengths until Kraft's sum is exact, then longest lengths to the rarest symbols; a lone symbol
//                gets a partner (symbol 0, or 1) so that every code is complete.  The header sends the 258 lengths plainly (code-length
//                symbols 0..15 only): on filtered photographs runs are rare, and plain lengths keep the header a sum.
//                A block whose dynamic form would take more than 8 * len + 35 bits is sent stored, so the stream bound is arithmetic.
//   checksums    Adler-32 of the filtered bytes and CRC-32 of each chunk, both as per-piece values and a combine step.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define Y2P_HD __host__ __device__
#else
#define Y2P_HD
#endif

namespace y2p {

constexpr int kBlockLog2 = 15;
constexpr uint32_t kBlock = 1u << kBlockLog2;   // input bytes per deflate block (32 KiB: profiles/r22_png_rates.txt; a stored block holds < 64 KiB)
constexpr int kLitSyms = 257, kEob = 256, kLitMaxLen = 15, kClSyms = 19, kClMaxLen = 7;
constexpr int kHdrBitsMax = 3 + 5 + 5 + 4 + 3 * kClSyms + (kLitSyms + 1) * kClMaxLen;   // 1880
constexpr int kHdrBytes = 256;                                                           // a block's header slot (dword multiple)
constexpr uint32_t kStoredSlack = 35;   // 3 header bits + LEN + NLEN: the least a stored block adds to its bytes
constexpr uint32_t kBlockBitsOver = 42; // ... and the most (7 bits of padding up to the byte)
static_assert(kBlock <= 65535, "a block must fit one stored block");
static_assert(kHdrBitsMax <= kHdrBytes * 8, "header slot");

// ---------------------------------------------------------------------------------------------------------------- sizes
Y2P_HD inline size_t n_blocks(size_t n) { return n ? (n + kBlock - 1) >> kBlockLog2 : 1; }
Y2P_HD inline uint32_t block_len(size_t n, size_t b) { return (uint32_t)(n - b * kBlock < kBlock ? n - b * kBlock : kBlock); }
// the most bytes the zlib stream of n input bytes takes: 2 header, every block stored at the worst alignment, 4 Adler-32
Y2P_HD inline size_t zlib_bound(size_t n) { return 2 + n + (n_blocks(n) * kBlockBitsOver + 7) / 8 + 4; }
Y2P_HD inline size_t filtered_bytes(int w, int h) { return (size_t)h * (1 + 3 * (size_t)w); }
constexpr size_t kPngIdatAt = 8 + 25 + 8;   // signature, IHDR chunk, IDAT's length and type: where the zlib stream starts
// ... of the PNG file of a w x h frame: signature, IHDR, IDAT, IEND
Y2P_HD inline size_t png_bound(int w, int h) { return kPngIdatAt + zlib_bound(filtered_bytes(w, h)) + 4 + 12; }

// ---------------------------------------------------------------------------------------------------------------- row filter
Y2P_HD inline int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// byte x under filter t; a: the byte a pixel to the left, b: above, c: above left
Y2P_HD inline uint8_t filter_value(int t, int x, int a, int b, int c)
{
    const int p = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(x - p);
}
// byte i of the row `cur` under filter t; up: the row above or nullptr (zeros)
Y2P_HD inline uint8_t filter_byte(int t, const uint8_t *cur, const uint8_t *up, int i)
{
    return filter_value(t, cur[i], i >= 3 ? cur[i - 3] : 0, up ? up[i] : 0, (up && i >= 3) ? up[i - 3] : 0);
}
Y2P_HD inline uint32_t filter_cost(uint8_t v) { return v < 128 ? v : 256u - v; }   // abs((int8_t)v)
Y2P_HD inline int filter_pick(const uint32_t *score)
{
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (score[t] < score[best]) best = t;
    return best;
}

// ---------------------------------------------------------------------------------------------------------------- code lengths
// every array the construction indexes by a variable lives here, so that the device keeps it in LDS and nothing spills to scratch
struct HuffScratch {
    uint32_t key[kLitSyms];          // count << 9 | symbol, of the symbols in use
    uint32_t wt[kLitSyms];           // inner nodes: weight, then depth
    uint16_t parent[2 * kLitSyms];   // node -> inner node; leaves 0 .. n - 1 in key order, inner nodes n .. 2 n - 2 in order of creation
    uint32_t count[17], next[17];    // codes per length, first code per length
    uint32_t ch[kClSyms];            // the code-length code's histogram
    uint8_t cl_len[kClSyms];
};

// keys of the symbols with a count, in symbol order; returns how many
Y2P_HD inline int used_keys(const uint32_t *hist, int nsym, uint32_t *key)
{
    int n = 0;
    for (int s = 0; s < nsym; ++s)
        if (hist[s]) key[n++] = (hist[s] << 9) | (uint32_t)s;
    return n;
}
// ascending; keys are distinct (the symbol is part of them), so every correct sort gives this order
Y2P_HD inline void sort_keys(uint32_t *key, int n)
{
    for (int i = 1; i < n; ++i) {
        const uint32_t k = key[i];
        int j = i;
        for (; j > 0 && key[j - 1] > k; --j) key[j] = key[j - 1];
        key[j] = k;
    }
}
// a lone symbol gets a partner of count 0 in front of it: symbol 0, or 1 if the lone one is 0
Y2P_HD inline int force_two(uint32_t *key, int n)
{
    if (n >= 2) return n;
    if (n == 1) { key[1] = key[0]; key[0] = (key[1] & 511u) == 0 ? 1u : 0u; }
    else { key[0] = 0; key[1] = 1; }
    return 2;
}
// sorted keys (n >= 2) -> len[symbol] (entries of unused symbols are not written), no length above maxlen
Y2P_HD inline void limited_lengths(HuffScratch &w, int n, int maxlen, uint8_t *len)
{
    int li = 0, ii = 0;
    for (int j = 0; j < n - 1; ++j) {   // two queues: leaves in key order, inner nodes in order of creation (weights never fall)
        uint32_t sum = 0;
        for (int k = 0; k < 2; ++k) {
            int id;
            if (li < n && (ii >= j || (w.key[li] >> 9) <= w.wt[ii])) { id = li; sum += w.key[li++] >> 9; }
            else { id = n + ii; sum += w.wt[ii++]; }
            w.parent[id] = (uint16_t)(n + j);
        }
        w.wt[j] = sum;
    }
    w.wt[n - 2] = 0;   // depths, root first: a parent is made after its children
    for (int j = n - 3; j >= 0; --j) w.wt[j] = w.wt[w.parent[n + j] - n] + 1;
    uint32_t *count = w.count;
    for (int l = 0; l <= maxlen; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t d = w.wt[w.parent[i] - n] + 1;
        ++count[d < (uint32_t)maxlen ? d : (uint32_t)maxlen];
    }
    uint32_t kraft = 0;
    for (int l = 1; l <= maxlen; ++l) kraft += count[l] << (maxlen - l);
    for (; kraft > (1u << maxlen); --kraft) {   // a code leaves the last level and becomes the sibling of one pushed a level down
        --count[maxlen];
        for (int l = maxlen - 1; l >= 1; --l)
            if (count[l]) { --count[l]; count[l + 1] += 2; break; }
    }
    int at = 0;
    for (int l = maxlen; l >= 1; --l)
        for (uint32_t c = 0; c < count[l]; ++c) len[w.key[at++] & 511u] = (uint8_t)l;
}
// hist[nsym] -> len[nsym] (zero for unused symbols); presorted: w.key already holds the n sorted keys (the wavefront's rank sort)
Y2P_HD inline void code_lengths(const uint32_t *hist, int nsym, int maxlen, HuffScratch &w, uint8_t *len, bool presorted = false, int n = 0)
{
    if (!presorted) { n = used_keys(hist, nsym, w.key); sort_keys(w.key, n); }
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    limited_lengths(w, force_two(w.key, n), maxlen, len);
}
// canonical codes (RFC 1951 3.2.2), bit-reversed for LSB-first packing: out[s] = code | len << 16
Y2P_HD inline void canonical_codes(const uint8_t *len, int nsym, HuffScratch &w, uint32_t *out)
{
    uint32_t *count = w.count, *next = w.next;
    for (int b = 0; b <= 16; ++b) count[b] = 0;
    for (int s = 0; s < nsym; ++s) ++count[len[s]];
    count[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= 15; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        uint32_t c = l ? next[l]++ : 0, r = 0;
        for (int i = 0; i < l; ++i) { r = (r << 1) | (c & 1u); c >>= 1; }
        out[s] = r | ((uint32_t)l << 16);
    }
}

// ---------------------------------------------------------------------------------------------------------------- block header
Y2P_HD inline int cl_order(int i)
{
    const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
struct BlockHeader {
    uint32_t cl[kClSyms];   // the code-length code: code | len << 16
    int n_cl;               // HCLEN + 4
    uint32_t hdr_bits, dyn_bits;
    bool stored;
};
// lit_len[257] and the block's histogram -> the code-length code, the header's and the block's size, stored or not
Y2P_HD inline void plan_header(const uint32_t *hist, const uint8_t *lit_len, uint32_t blen, HuffScratch &w, BlockHeader *h)
{
    uint32_t *ch = w.ch;
    uint8_t *cl_len = w.cl_len;
    for (int l = 0; l < kClSyms; ++l) ch[l] = 0;
    for (int s = 0; s < kLitSyms; ++s) ++ch[lit_len[s]];
    ++ch[0];   // the one distance code, of zero bits
    code_lengths(ch, kClSyms, kClMaxLen, w, cl_len);
    canonical_codes(cl_len, kClSyms, w, h->cl);
    h->n_cl = 4;
    for (int i = 4; i < kClSyms; ++i)
        if (cl_len[cl_order(i)]) h->n_cl = i + 1;
    h->hdr_bits = 17 + 3 * (uint32_t)h->n_cl;
    for (int l = 0; l <= kLitMaxLen; ++l) h->hdr_bits += ch[l] * cl_len[l];
    h->dyn_bits = h->hdr_bits;
    for (int s = 0; s < kLitSyms; ++s) h->dyn_bits += hist[s] * lit_len[s];
    h->stored = h->dyn_bits > 8 * blen + kStoredSlack;
}
// the dynamic block's header through W::put(value, bits <= 16)
template <class W>
Y2P_HD inline void write_header(W &out, bool bfinal, const uint8_t *lit_len, const BlockHeader &h)
{
    out.put(bfinal ? 1u : 0u, 1);
    out.put(2u, 2);
    out.put(0u, 5);   // HLIT: 257 codes
    out.put(0u, 5);   // HDIST: 1 code
    out.put((uint32_t)h.n_cl - 4u, 4);
    for (int i = 0; i < h.n_cl; ++i) out.put(h.cl[cl_order(i)] >> 16, 3);
    for (int s = 0; s < kLitSyms; ++s) out.put(h.cl[lit_len[s]] & 0xffffu, (int)(h.cl[lit_len[s]] >> 16));
    out.put(h.cl[0] & 0xffffu, (int)(h.cl[0] >> 16));
}
// bits a block takes when it starts at bit `at` of the deflate data
Y2P_HD inline uint64_t block_bits(uint64_t at, bool stored, uint32_t dyn_bits, uint32_t blen)
{
    return stored ? 3 + ((0 - (at + 3)) & 7) + 32 + 8 * (uint64_t)blen : dyn_bits;
}
// LSB-first bits into bytes, one after the other (the host's stream; a block's header slot on the device)
struct ByteBits {
    uint8_t *p;
    size_t n = 0;
    uint64_t acc = 0;
    int fill = 0;
    Y2P_HD explicit ByteBits(uint8_t *dst) : p(dst) {}
    Y2P_HD void put(uint32_t v, int bits)
    {
        acc |= (uint64_t)v << fill;
        for (fill += bits; fill >= 8; fill -= 8, acc >>= 8) p[n++] = (uint8_t)acc;
    }
    Y2P_HD void align() { if (fill) { p[n++] = (uint8_t)acc; acc = 0; fill = 0; } }
};

// ---------------------------------------------------------------------------------------------------------------- checksums
constexpr uint32_t kAdlerMod = 65521, kCrcPoly = 0xEDB88320u;
// Adler-32 by pieces: a piece of len bytes d[i] gives A = sum d[i] and B = sum (len - i) d[i], both mod 65521; appended to a state:
Y2P_HD inline void adler_append(uint32_t &a, uint32_t &b, uint32_t pa, uint32_t pb, uint32_t len)
{
    b = (uint32_t)((b + (uint64_t)(len % kAdlerMod) * a + pb) % kAdlerMod);
    a = (a + pa) % kAdlerMod;
}
// CRC-32 by pieces.  raw(M): the register after M from a zero register, no final inversion; then raw(A B) = raw(A) x^(8 |B|) + raw(B)
// and crc(M) = ~(raw(M) + 0xffffffff x^(8 |M|)), in GF(2)[x] mod P, reflected (bit 31 is x^0).
Y2P_HD inline uint32_t crc_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1u) ? kCrcPoly : 0u);
    return i;
}
Y2P_HD inline uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}
Y2P_HD inline uint32_t crc_xpow8(uint64_t n)   // x^(8 n) mod P
{
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}
Y2P_HD inline uint32_t crc_raw_bytes(uint32_t c, const uint8_t *p, size_t n)   // table-free; for the few bytes around the payload
{
    for (size_t i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
    return c;
}
Y2P_HD inline uint32_t crc_finish(uint32_t raw, uint64_t len) { return ~(raw ^ crc_mul(0xffffffffu, crc_xpow8(len))); }

// ---------------------------------------------------------------------------------------------------------------- framing
Y2P_HD inline void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
// everything of the file in front of the zlib stream (kPngIdatAt bytes): signature, IHDR with its CRC, IDAT's length and type
Y2P_HD inline void png_head(uint8_t *p, int w, int h, size_t zlib_bytes)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) p[i] = sig[i];
    put_be32(p + 8, 13);
    p[12] = 'I'; p[13] = 'H'; p[14] = 'D'; p[15] = 'R';
    put_be32(p + 16, (uint32_t)w);
    put_be32(p + 20, (uint32_t)h);
    p[24] = 8; p[25] = 2; p[26] = 0; p[27] = 0; p[28] = 0;   // 8 bits, RGB, deflate, adaptive filters, no interlace
    put_be32(p + 29, crc_finish(crc_raw_bytes(0, p + 12, 17), 17));
    put_be32(p + 33, (uint32_t)zlib_bytes);
    p[37] = 'I'; p[38] = 'D'; p[39] = 'A'; p[40] = 'T';
}
// ... and behind the deflate data (kPngTail bytes): the zlib stream's Adler-32, IDAT's CRC from raw(the deflate data), then IEND.
// The zlib stream is 78 01, the data, Adler-32.
constexpr size_t kPngTail = 4 + 4 + 12;
Y2P_HD inline void png_tail(uint8_t *p, uint32_t raw_data, size_t data_bytes, uint32_t adler)
{
    const uint8_t pre[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    put_be32(p, adler);
    const uint32_t raw = crc_mul(crc_raw_bytes(0, pre, 6), crc_xpow8(data_bytes + 4)) ^ crc_mul(raw_data, crc_xpow8(4)) ^ crc_raw_bytes(0, p, 4);
    put_be32(p + 4, crc_finish(raw, data_bytes + 10));
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) p[8 + i] = iend[i];
}

}  // namespace y2p
