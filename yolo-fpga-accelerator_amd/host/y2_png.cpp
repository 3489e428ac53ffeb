// y2_png.cpp -- the annotated frame as a PNG file on the host: csrc/png_huff.hpp (the format's one statement) run front to back.
// zlib_huff is what yolo2_hip_zlib_huff produces on the GPU, byte for byte (tests/test_gpu_png.py).
#include <cstring>
#include <vector>

#include "../csrc/png_huff.hpp"
#include "y2_host.hpp"

namespace y2h {

namespace {
// the zlib stream of in[0 .. n) at out (zlib_bound(n) bytes at least); returns its length; raw: raw CRC-32 of the deflate data
size_t zlib_huff_into(const uint8_t *in, size_t n, uint8_t *out, uint32_t *raw_crc, size_t *data_bytes)
{
    out[0] = 0x78; out[1] = 0x01;
    y2p::ByteBits bits(out + 2);
    y2p::HuffScratch scratch;
    uint32_t adler_a = 1, adler_b = 0;
    const size_t nb = y2p::n_blocks(n);
    for (size_t b = 0; b < nb; ++b) {
        const uint8_t *d = in + b * y2p::kBlock;
        const uint32_t len = y2p::block_len(n, b);
        uint32_t hist[y2p::kLitSyms] = {0}, codes[y2p::kLitSyms];
        uint64_t pa = 0, pb = 0;
        for (uint32_t i = 0; i < len; ++i) { ++hist[d[i]]; pa += d[i]; pb += (uint64_t)(len - i) * d[i]; }
        y2p::adler_append(adler_a, adler_b, (uint32_t)(pa % y2p::kAdlerMod), (uint32_t)(pb % y2p::kAdlerMod), len);
        hist[y2p::kEob] = 1;
        uint8_t lit_len[y2p::kLitSyms];
        y2p::code_lengths(hist, y2p::kLitSyms, y2p::kLitMaxLen, scratch, lit_len);
        y2p::BlockHeader h;
        y2p::plan_header(hist, lit_len, len, scratch, &h);
        const bool last = b + 1 == nb;
        if (h.stored) {
            bits.put(last ? 1u : 0u, 3);
            bits.align();
            bits.put(len, 16);
            bits.put(~len & 0xffffu, 16);
            for (uint32_t i = 0; i < len; ++i) bits.put(d[i], 8);
            continue;
        }
        y2p::canonical_codes(lit_len, y2p::kLitSyms, scratch, codes);
        y2p::write_header(bits, last, lit_len, h);
        for (uint32_t i = 0; i < len; ++i) bits.put(codes[d[i]] & 0xffffu, (int)(codes[d[i]] >> 16));
        bits.put(codes[y2p::kEob] & 0xffffu, (int)(codes[y2p::kEob] >> 16));
    }
    bits.align();
    y2p::put_be32(out + 2 + bits.n, (adler_b << 16) | adler_a);
    if (raw_crc) {   // by the pieces the device uses: bytewise from a zero register
        uint32_t c = 0, table[256];
        for (uint32_t i = 0; i < 256; ++i) table[i] = y2p::crc_table_entry(i);
        for (size_t i = 0; i < bits.n; ++i) c = table[(c ^ out[2 + i]) & 255u] ^ (c >> 8);
        *raw_crc = c;
        *data_bytes = bits.n;
    }
    return 2 + bits.n + 4;
}
}  // namespace

size_t zlib_huff_bound(size_t n) { return y2p::zlib_bound(n); }

long zlib_huff(const uint8_t *in, size_t n, uint8_t *out, size_t cap)
{
    if ((n && !in) || (cap && !out)) return -1;
    std::vector<uint8_t> z(y2p::zlib_bound(n));
    const size_t size = zlib_huff_into(in, n, z.data(), nullptr, nullptr);
    if (cap) memcpy(out, z.data(), size < cap ? size : cap);
    return (long)size;
}

static bool png_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 && y2p::png_bound(w, h) < ((size_t)1 << 31); }

size_t png_rgb24_bound(int w, int h) { return png_size_ok(w, h) ? y2p::png_bound(w, h) : 0; }

long write_png_rgb24(const uint8_t *rgb, int w, int h, uint8_t *out, size_t cap)
{
    if (!rgb || !png_size_ok(w, h) || (cap && !out)) return -1;
    const int rb = 3 * w;
    std::vector<uint8_t> filt(y2p::filtered_bytes(w, h)), png(y2p::png_bound(w, h));
    for (int y = 0; y < h; ++y) {
        const uint8_t *cur = rgb + (size_t)y * rb, *up = y ? cur - rb : nullptr;
        uint32_t score[5] = {0};
        for (int t = 0; t < 5; ++t)
            for (int i = 0; i < rb; ++i) score[t] += y2p::filter_cost(y2p::filter_byte(t, cur, up, i));
        const int t = y2p::filter_pick(score);
        uint8_t *row = filt.data() + (size_t)y * (rb + 1);
        row[0] = (uint8_t)t;
        for (int i = 0; i < rb; ++i) row[1 + i] = y2p::filter_byte(t, cur, up, i);
    }
    uint32_t raw = 0;
    size_t data_bytes = 0;
    const size_t zbytes = zlib_huff_into(filt.data(), filt.size(), png.data() + y2p::kPngIdatAt, &raw, &data_bytes);
    y2p::png_head(png.data(), w, h, zbytes);
    uint32_t adler = 0;
    for (int i = 0; i < 4; ++i) adler = (adler << 8) | png[y2p::kPngIdatAt + zbytes - 4 + i];
    y2p::png_tail(png.data() + y2p::kPngIdatAt + zbytes - 4, raw, data_bytes, adler);
    const size_t size = y2p::kPngIdatAt + zbytes + 16;
    if (cap) memcpy(out, png.data(), size < cap ? size : cap);
    return (long)size;
}

}  // namespace y2h
