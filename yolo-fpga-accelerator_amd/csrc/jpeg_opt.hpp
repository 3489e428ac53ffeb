// jpeg_opt.hpp -- mode optimize = 1 of the JPEG stream (jpeg_tables.hpp includes this file at its end; include that one): the four
// Huffman tables and the DHT segment are made from the frame's own symbol counts, libjpeg's -optimize.  Coefficients, MCU order,
// restart handling and stuffing are the mode's without it.  Plain C++: the host encoder (host/y2_jpeg.cpp) and k_jpeg_opt_tables
// (kernels_jpeg.hpp) compile this one statement, as png_huff.hpp is for PNG, and the tree is that file's.
//
//   symbols      what the encoder emits: per block the category of its DC difference (predictor as the mode has it), per non-zero AC
//                coefficient (run & 15) << 4 | category, 0xF0 per sixteen zeros in front of one, 0x00 when coefficient 63 is zero.
//                Luma blocks count into the luma tables, Cb and Cr into the chroma tables: kOptHistBins counts, opt_hist_at(table).
//   lengths      y2p::limited_lengths over the used symbols and one reserved symbol (value 256, count 0), sorted by (count, symbol):
//                the reserved one is the rarest, so it gets the longest length, and the largest value, so it is last in code order -
//                it takes the all-ones code word, which T.81 keeps from every real symbol.  At most 16 bits (AC) and 11 (DC: a DC code
//                and its value stay within 22 bits, kBlockBitsMax holds and no work area changes).  A lone symbol gets length 1.
//   code words   canonical, T.81 Annex C: by length, then by symbol value; HUFFVAL lists the used symbols in that order.
//   fallback     cost = the scan's code bits (sum of count * length) + 8 * the DHT payload's bytes, for the frame's tables and for the
//                standard ones; the frame's four tables are used only when their cost is strictly smaller.  A table whose counts add
//                up to kOptCountLimit or more (the sort key holds 23 bits of count) is not built: such a frame falls back too.  A
//                frame that falls back is the mode's standard stream, byte for byte.
//   header       the standard one with the DHT segment's payload replaced: opt_header_byte, opt_header_len bytes (<= the standard's).
#pragma once
#include "png_huff.hpp"

namespace y2j {

constexpr int kOptHistBins = 12 + 12 + 256 + 256, kOptReserved = 256;
constexpr uint32_t kOptCountLimit = 1u << 23;
constexpr int kHeaderDhtAt = 173;                                    // FF C4, length, then the payload: id, BITS[16], HUFFVAL per table
constexpr int kDhtStdPayload = 4 * 17 + 12 + 162 + 12 + 162;
constexpr int kOptHeaderSlot = 640;                                  // room for a frame's header (at most header_bytes(restart))
static_assert(kHeaderDhtAt + 4 + kDhtStdPayload + 14 == kHeaderBytes, "header layout");

// tables in the DHT segment's order, which is the order of kDcLuma .. kAcChroma
Y2T_HD inline int opt_hist_at(int t) { return t == kDcLuma ? 0 : t == kDcChroma ? 12 : t == kAcLuma ? 24 : 280; }
Y2T_HD inline int opt_syms(int t) { return (t & 1) ? 256 : 12; }
Y2T_HD inline int opt_maxlen(int t) { return (t & 1) ? 16 : 11; }
Y2T_HD inline int opt_dht_id(int t) { return ((t & 1) << 4) | (t >> 1); }

// every array the construction indexes by a variable (LDS on the device)
struct OptScratch {
    y2p::HuffScratch h;
    uint8_t len[kOptReserved + 4];   // per symbol, the reserved one included; 0: unused
    uint32_t first[17], at[17];      // per length: the first code word, the first place in HUFFVAL (h.count: BITS)
};

// h.key holds the n >= 2 sorted keys (count << 9 | symbol), the reserved symbol's among them -> len
Y2T_HD inline void opt_lengths(OptScratch &w, int n, int maxlen) { y2p::limited_lengths(w.h, n, maxlen, w.len); }
// len -> h.count[1..16] (BITS), first, at; returns the number of real symbols in use
Y2T_HD inline int opt_canon_prepare(OptScratch &w, int nsym)
{
    uint32_t *count = w.h.count;
    for (int l = 0; l <= 16; ++l) count[l] = 0;
    for (int s = 0; s < nsym; ++s) ++count[w.len[s]];
    count[0] = 0;
    uint32_t code = 0, at = 0;
    for (int l = 1; l <= 16; ++l) {
        w.first[l] = code;
        w.at[l] = at;
        code = (code + count[l]) << 1;
        at += count[l];
    }
    return (int)at;
}
// symbol s (len[s] != 0): its code word | length << 16, and its place in HUFFVAL
Y2T_HD inline uint32_t opt_canon_symbol(const OptScratch &w, int s, int *place)
{
    const int l = w.len[s];
    uint32_t r = 0;
    for (int q = 0; q < s; ++q) r += w.len[q] == l;
    *place = (int)(w.at[l] + r);
    return (w.first[l] + r) | ((uint32_t)l << 16);
}

Y2T_HD inline int opt_header_len(int dht_payload, int restart) { return header_bytes(restart) - kDhtStdPayload + dht_payload; }
// byte i of the header with the DHT payload `dht` (dht_payload bytes); base: Tables::header
Y2T_HD inline uint8_t opt_header_byte(const uint8_t *base, int i, int w, int h, int subsample, int restart, const uint8_t *dht, int dht_payload)
{
    const int j = i - (kHeaderDhtAt + 4);
    if (j >= dht_payload) return header_byte(base, i - dht_payload + kDhtStdPayload, w, h, subsample, restart);
    if (j >= 0) return dht[j];
    if (j == -2) return (uint8_t)((dht_payload + 2) >> 8);
    if (j == -1) return (uint8_t)(dht_payload + 2);
    return header_byte(base, i, w, h, subsample, restart);
}

// ---- the host's side: one frame, serially
struct OptTables {
    uint32_t code[4][256];
    uint8_t header[kOptHeaderSlot];
    int head_len;
    bool used;   // false: the standard tables and header (the fallback)
};
inline void opt_build(const uint32_t *hist, const Tables &std_t, int w, int h, int subsample, int restart, OptTables *o)
{
    OptScratch s;
    uint8_t dht[kDhtStdPayload];
    int payload = 0;
    unsigned long long cost_opt = 0, cost_std = 0;
    bool ok = true;
    std::memset(o->code, 0, sizeof(o->code));
    for (int t = 0; t < 4 && ok; ++t) {
        const uint32_t *ht = hist + opt_hist_at(t);
        const int nsym = opt_syms(t);
        unsigned long long total = 0;
        for (int q = 0; q < nsym; ++q) total += ht[q];
        if (total >= kOptCountLimit) { ok = false; break; }
        for (int q = 0; q <= kOptReserved; ++q) s.len[q] = 0;
        s.h.key[0] = (uint32_t)kOptReserved;
        const int n = 1 + y2p::used_keys(ht, nsym, s.h.key + 1);
        y2p::sort_keys(s.h.key, n);
        if (n >= 2) opt_lengths(s, n, opt_maxlen(t));
        const int used = opt_canon_prepare(s, nsym);
        if (payload + 17 + used > kDhtStdPayload) { ok = false; break; }   // (more symbols than T.81 has: not from 8-bit pixels)
        uint8_t *seg = dht + payload;
        seg[0] = (uint8_t)opt_dht_id(t);
        for (int l = 1; l <= 16; ++l) seg[l] = (uint8_t)s.h.count[l];
        for (int q = 0; q < nsym; ++q) {
            if (!s.len[q]) continue;
            int place;
            o->code[t][q] = opt_canon_symbol(s, q, &place);
            seg[17 + place] = (uint8_t)q;
            cost_opt += (unsigned long long)ht[q] * s.len[q];
            cost_std += (unsigned long long)ht[q] * (std_t.code[t][q] >> 16);
        }
        payload += 17 + used;
    }
    o->used = ok && cost_opt + 8ull * (unsigned)payload < cost_std + 8ull * kDhtStdPayload;
    if (!o->used) {
        std::memcpy(o->code, std_t.code, sizeof(o->code));
        o->head_len = header_bytes(restart);
        for (int i = 0; i < o->head_len; ++i) o->header[i] = header_byte(std_t.header, i, w, h, subsample, restart);
        return;
    }
    o->head_len = opt_header_len(payload, restart);
    for (int i = 0; i < o->head_len; ++i) o->header[i] = opt_header_byte(std_t.header, i, w, h, subsample, restart, dht, payload);
}

}  // namespace y2j
