// jpeg_tables.hpp -- everything of the annotated frame's JPEG stream that does not depend on the pixels: the scaled quantisation
// tables, the reciprocal table of the float AAN transform, the Huffman code words and the 607-byte header.  Plain C++ (no HIP): the
// host encoder (host/y2_jpeg.cpp) and the device encoder's host side (csrc/yolo2_jpeg.hip) both make their tables here, so the GPU
// never computes one.  The stream is the one the reference's MJPEG streamer sends (stb_image_write v1.09 through
// linux_app/src/yolo2_mjpeg_server.c:221-238): baseline, three components without subsampling, the typical tables of ITU-T T.81
// Annex K, no restart markers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace y2j {

constexpr int kHeaderBytes = 607;
// A block's code words are at most 22 + 63 * 26 bits.  The transform and fdtbl together are the DCT of T.81 A.3.3 divided by the
// table entry q >= 1: F(u,v) = 1/4 C(u) C(v) sum f(x,y) cos((2x+1) u pi/16) cos((2y+1) v pi/16), with |f| <= 128 for 8-bit input
// (level-shifted luma in [-128, 127], chroma within +-127.5).
//   DC: F(0,0) = sum f / 8 lies in [-1024, 1020] (luma mean in [-128, 127], chroma mean within +-127.5), so the difference of two
//       DC levels is at most 2044 < 2^11 in magnitude: category <= 11, a code of at most 11 bits (the chroma table's longest) plus
//       11 value bits = 22.
//   AC: with S(u) = sum_x |cos((2x+1) u pi/16)| (S(0) = 8, S(4) = 5.657, the others 5.13 .. 5.23), |F(u,v)| <= 32 C(u) C(v) S(u) S(v)
//       for |f| <= 128: 32 * 5.657^2 = 1024 at (4,4) and 32 * 0.7071 * 8 * 5.657 = 1024 at (0,4) / (4,0), reached only with f = -128
//       on one half of the pixels and +128 on the other.  8-bit input gives at most +127.5 there, which scales the bound to
//       1024 * 127.75 / 128 = 1022; fp32 rounding moves that by far less than 1, and the +-0.5 before truncation keeps the level at
//       or below 1022 < 2^10: category <= 10, a code of at most 16 bits plus 10 value bits = 26, and 63 of them.  A zero coefficient
//       only shortens the block (sixteen of them share one 11-bit code), and the end-of-block code is written only when
//       coefficient 63 is zero, in place of at least one 26-bit worst case.
constexpr int kBlockBitsMax = 22 + 63 * 26;

// natural (row-major) index -> position in the zigzag sequence
constexpr uint8_t kZigzag[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
// T.81 tables K.1 and K.2, natural order
constexpr uint8_t kQuantLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                    14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQuantChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// T.81 tables K.3 - K.6: codes per length 1..16, then the symbols in code order
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcSymbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaSymbols[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaSymbols[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

enum { kDcLuma = 0, kAcLuma = 1, kDcChroma = 2, kAcChroma = 3 };

// Where the frame's size sits in the header: SOF0's height and width, two big-endian bytes each.
constexpr int kHeaderHeightAt = 159, kHeaderWidthAt = 161;

struct Tables {
    float fdtbl[2][64];      // [0] luma, [1] chroma: what a transformed coefficient (natural index) is multiplied by before rounding
    uint32_t code[4][256];   // kDcLuma .. kAcChroma: symbol -> code word | length << 16 (0: the symbol has no code)
    uint8_t header[608];     // SOI .. SOS, kHeaderBytes of it, for a 0 x 0 frame (patch kHeaderHeightAt / kHeaderWidthAt)
};

// the streamer's rule: 1..100 (0 is 1, not the writer's own default)
inline int clamp_quality(int q) { return q < 1 ? 1 : q > 100 ? 100 : q; }

// canonical code words of one table (T.81 Annex C): symbols in order, codes counting up within a length, doubled between lengths
inline void huffman_codes(const uint8_t *bits, const uint8_t *symbols, uint32_t *code)
{
    uint32_t next = 0;
    int at = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) code[symbols[at++]] = next++ | ((uint32_t)len << 16);
        next <<= 1;
    }
}

inline void make_tables(int quality, Tables *t)
{
    std::memset(t, 0, sizeof(*t));
    const int q = clamp_quality(quality), scale = q < 50 ? 5000 / q : 200 - 2 * q;
    uint8_t qt[2][64];   // scaled tables, natural index
    for (int i = 0; i < 64; ++i) {
        const int y = (kQuantLuma[i] * scale + 50) / 100, c = (kQuantChroma[i] * scale + 50) / 100;
        qt[0][i] = (uint8_t)(y < 1 ? 1 : y > 255 ? 255 : y);
        qt[1][i] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    // the AAN transform leaves row r / column c scaled by these; the quantiser's division and this scale are one multiplication
    const float aan[8] = {1.0f * 2.828427125f,         1.387039845f * 2.828427125f, 1.306562965f * 2.828427125f, 1.175875602f * 2.828427125f,
                          1.0f * 2.828427125f,         0.785694958f * 2.828427125f, 0.541196100f * 2.828427125f, 0.275899379f * 2.828427125f};
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c)
            for (int k = 0; k < 2; ++k) {
                const float a = (float)qt[k][r * 8 + c] * aan[r];
                const float b = a * aan[c];
                t->fdtbl[k][r * 8 + c] = 1.0f / b;
            }
    huffman_codes(kDcLumaBits, kDcSymbols, t->code[kDcLuma]);
    huffman_codes(kAcLumaBits, kAcLumaSymbols, t->code[kAcLuma]);
    huffman_codes(kDcChromaBits, kDcSymbols, t->code[kDcChroma]);
    huffman_codes(kAcChromaBits, kAcChromaSymbols, t->code[kAcChroma]);

    uint8_t *p = t->header;
    auto put = [&](std::initializer_list<int> bytes) { for (int b : bytes) *p++ = (uint8_t)b; };
    auto put_n = [&](const uint8_t *src, int n) { std::memcpy(p, src, (size_t)n); p += n; };
    put({0xFF, 0xD8});                                                                          // SOI
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});                 // APP0: JFIF 1.1, aspect 1:1, no thumbnail
    put({0xFF, 0xDB, 0, 2 + 2 * 65});                                                           // DQT: both tables, 8 bit, zigzag order
    for (int k = 0; k < 2; ++k) {
        *p++ = (uint8_t)k;
        for (int i = 0; i < 64; ++i) p[kZigzag[i]] = qt[k][i];
        p += 64;
    }
    put({0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});             // SOF0: 8 bit, h, w, Y / Cb / Cr all 1x1
    put({0xFF, 0xC4, 0x01, 0xA2});                                                              // DHT: four tables
    const struct { int id; const uint8_t *bits, *sym; int n; } ht[4] = {{0x00, kDcLumaBits, kDcSymbols, 12}, {0x10, kAcLumaBits, kAcLumaSymbols, 162},
                                                                        {0x01, kDcChromaBits, kDcSymbols, 12}, {0x11, kAcChromaBits, kAcChromaSymbols, 162}};
    for (const auto &h : ht) {
        *p++ = (uint8_t)h.id;
        put_n(h.bits, 16);
        put_n(h.sym, h.n);
    }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});                           // SOS: whole spectrum, one scan
}

inline void header_for(const Tables &t, int w, int h, uint8_t *out)
{
    std::memcpy(out, t.header, kHeaderBytes);
    out[kHeaderHeightAt] = (uint8_t)(h >> 8); out[kHeaderHeightAt + 1] = (uint8_t)h;
    out[kHeaderWidthAt] = (uint8_t)(w >> 8);  out[kHeaderWidthAt + 1] = (uint8_t)w;
}

// the most bytes a w x h stream can take: header, every block at kBlockBitsMax with every byte stuffed, EOI
inline size_t stream_bound(int w, int h)
{
    const size_t blocks = 3 * (size_t)((w + 7) / 8) * (size_t)((h + 7) / 8);
    return (size_t)kHeaderBytes + 2 * ((blocks * kBlockBitsMax + 7) / 8) + 2;
}

}  // namespace y2j
