// y2_jpeg.cpp -- write_jpg_rgb24: an RGB24 frame as the JPEG stream the reference's MJPEG streamer sends for it
// (stbi_write_jpg_to_func with 3 components, linux_app/src/yolo2_mjpeg_server.c:221-238; the writer is stb_image_write v1.09), byte
// for byte.  tests/golden/jpeg.npz, made by the compiled reference, pins it; the GPU encoder (csrc/yolo2_jpeg.hip) is tested against
// this function.  What decides bytes: fp32 throughout with one rounding per operation (this file is compiled without contraction),
// the operation order of the colour transform and of the AAN butterflies, rounding by adding +-0.5 and truncating.
#include "y2_host.hpp"

#include "../csrc/jpeg_tables.hpp"

namespace y2h {
namespace {

// one 8-point pass of the AAN forward transform (Arai, Agui, Nakajima 1988; the float form of the IJG's jfdctflt), in place with a stride
void aan_pass(float *d, int s)
{
    const float a0 = d[0] + d[7 * s], a7 = d[0] - d[7 * s], a1 = d[s] + d[6 * s], a6 = d[s] - d[6 * s];
    const float a2 = d[2 * s] + d[5 * s], a5 = d[2 * s] - d[5 * s], a3 = d[3 * s] + d[4 * s], a4 = d[3 * s] - d[4 * s];
    // even half
    const float e0 = a0 + a3, e3 = a0 - a3, e1 = a1 + a2, e2 = a1 - a2;
    d[0] = e0 + e1;
    d[4 * s] = e0 - e1;
    const float r = (e2 + e3) * 0.707106781f;
    d[2 * s] = e3 + r;
    d[6 * s] = e3 - r;
    // odd half
    const float o0 = a4 + a5, o1 = a5 + a6, o2 = a6 + a7;
    const float k = (o0 - o2) * 0.382683433f;
    const float p = o0 * 0.541196100f + k, q = o2 * 1.306562965f + k, m = o1 * 0.707106781f;
    const float s0 = a7 + m, s1 = a7 - m;
    d[5 * s] = s1 + p;
    d[3 * s] = s1 - p;
    d[s] = s0 + q;
    d[7 * s] = s0 - q;
}

// magnitude category of v (0 for 0) and the value bits that follow the code: v itself, or v - 1 for a negative v, in `cat` bits
int category(int v, uint32_t *extra)
{
    int mag = v < 0 ? -v : v, cat = 0;
    while (mag) { ++cat; mag >>= 1; }
    *extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    return cat;
}

// the output: counts every byte, stores those below the capacity
struct Sink {
    uint8_t *out;
    size_t cap, n = 0;
    uint32_t acc = 0;   // pending bits, the oldest highest
    int have = 0;
    void byte(uint8_t b) { if (n < cap) out[n] = b; ++n; }
    void bits(uint32_t v, int len)   // most significant first; a 0xFF byte of the scan is followed by a zero byte
    {
        for (int i = len - 1; i >= 0; --i) {
            acc = (acc << 1) | ((v >> i) & 1u);
            if (++have == 8) {
                byte((uint8_t)acc);
                if ((acc & 255u) == 255u) byte(0);
                acc = 0;
                have = 0;
            }
        }
    }
    void code(uint32_t c) { bits(c & 0xffffu, (int)(c >> 16)); }
};

// transform, quantise and code one block; returns its DC level (the next block's predictor)
int put_block(Sink &s, float *blk, const float *fdtbl, int pred, const uint32_t *dc, const uint32_t *ac)
{
    for (int r = 0; r < 8; ++r) aan_pass(blk + 8 * r, 1);
    for (int c = 0; c < 8; ++c) aan_pass(blk + c, 8);
    int zz[64];
    for (int i = 0; i < 64; ++i) {
        const float v = blk[i] * fdtbl[i];
        zz[y2j::kZigzag[i]] = (int)(v < 0 ? v - 0.5f : v + 0.5f);
    }
    uint32_t extra;
    int cat = category(zz[0] - pred, &extra);
    s.code(dc[cat]);
    s.bits(extra, cat);
    int run = 0;
    for (int i = 1; i < 64; ++i) {
        if (zz[i] == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) s.code(ac[0xF0]);   // sixteen zeros
        cat = category(zz[i], &extra);
        s.code(ac[(run << 4) | cat]);
        s.bits(extra, cat);
        run = 0;
    }
    if (run) s.code(ac[0x00]);   // end of block, unless coefficient 63 closed it
    return zz[0];
}

}  // namespace

size_t jpg_rgb24_bound(int w, int h) { return w >= 1 && h >= 1 && w <= 65535 && h <= 65535 ? y2j::stream_bound(w, h) : 0; }

long write_jpg_rgb24(const uint8_t *rgb, int w, int h, int quality, uint8_t *out, size_t cap)
{
    if (!rgb || w < 1 || h < 1 || w > 65535 || h > 65535 || (cap && !out)) return -1;
    y2j::Tables t;
    y2j::make_tables(quality, &t);
    Sink s{out, cap};
    uint8_t head[y2j::kHeaderBytes];
    y2j::header_for(t, w, h, head);
    for (uint8_t b : head) s.byte(b);
    int pred[3] = {0, 0, 0};
    float Y[64], U[64], V[64];
    for (int y0 = 0; y0 < h; y0 += 8)
        for (int x0 = 0; x0 < w; x0 += 8) {
            for (int r = 0; r < 8; ++r) {
                const uint8_t *row = rgb + (size_t)(y0 + r < h ? y0 + r : h - 1) * w * 3;   // edge pixels are repeated
                for (int c = 0; c < 8; ++c) {
                    const uint8_t *px = row + (size_t)(x0 + c < w ? x0 + c : w - 1) * 3;
                    const float R = px[0], G = px[1], B = px[2];
                    Y[r * 8 + c] = 0.299f * R + 0.587f * G + 0.114f * B - 128;
                    U[r * 8 + c] = -0.16874f * R - 0.33126f * G + 0.5f * B;
                    V[r * 8 + c] = 0.5f * R - 0.41869f * G - 0.08131f * B;
                }
            }
            pred[0] = put_block(s, Y, t.fdtbl[0], pred[0], t.code[y2j::kDcLuma], t.code[y2j::kAcLuma]);
            pred[1] = put_block(s, U, t.fdtbl[1], pred[1], t.code[y2j::kDcChroma], t.code[y2j::kAcChroma]);
            pred[2] = put_block(s, V, t.fdtbl[1], pred[2], t.code[y2j::kDcChroma], t.code[y2j::kAcChroma]);
        }
    if (s.have) s.bits(0x7fu, 8 - s.have);   // the last byte's free bits are ones
    s.byte(0xFF);
    s.byte(0xD9);   // EOI
    return (long)s.n;
}

}  // namespace y2h
