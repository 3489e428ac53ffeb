// draw_list.hpp -- the annotated frame of the reference's camera / video loop as data: what yolo2_draw_detections_rgb24
// (linux_app/src/yolo2_draw.c:276-369) paints for one detection record, worked out as one DrawItem.  Plain C++, no HIP includes:
// the host restatement (host/y2_host.cpp, y2h::draw_detections_rgb24) paints items one after the other like the reference does, and
// the GPU entries (yolo2_draw.hip) upload them for k_annotate_batch (kernels_draw.hpp), which asks per pixel which item painted last.
// Corner casts and the "%s %.2f" text are made here, by the host's own arithmetic and snprintf, so both are the reference's by
// construction (draw_make_item).  The loop entry makes the same items on the device (k_draw_items): its route, draw_item_from_record,
// shares the geometry with draw_make_item and formats the text in integers (draw_text_glyphs; tests/test_loop_host.py holds the two
// texts together).  The font and the palette are this project's own tables, recovered from what the compiled reference renders
// (tests/golden/make_draw_golden.py renders every glyph; tests/test_draw_host.py compares).
#pragma once
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

// The record -> item arithmetic and the text formatter below compile for the device too (k_draw_items, kernels_draw.hpp) and stay
// plain C++ for g++: one source serves the kernel, libyolo2_host.so and the CPU tests.
#if defined(__HIPCC__)
#define Y2D_HD __host__ __device__
#else
#define Y2D_HD
#endif

namespace y2d {

// yolo2_hip_det's layout (include/yolo2_hip.h; yolo2_draw.hip asserts the sizes agree), YOLO2_DETS_BEST_CLASS form: one per detection
struct DrawDet {
    int frame, det, cls;
    float prob, x, y, w, h;
};

constexpr int kDrawMaxText = 127;   // "%s %.2f" into char[128]
constexpr int kDrawGlyphs = 38;
constexpr int kDrawScale = 2, kDrawCell = 6 * kDrawScale, kDrawGlyphH = 7 * kDrawScale, kDrawPad = 2, kDrawThick = 2;

// 5 x 7 glyphs, one 35-bit word each: bit 5 * row + column, column 0 on the left.  Order: space . 0-9 a-z (A-Z use a-z's)
constexpr uint64_t kDrawFont[kDrawGlyphs] = {
    0x000000000ull, 0x108000000ull, 0x3a318c62eull, 0x3884210c4ull, 0x7c444422eull, 0x3a306422eull, 0x211f4a988ull, 0x3a3083c3full,
    0x3a317844cull, 0x08422221full, 0x3a317462eull, 0x1910f462eull, 0x4631fc62eull, 0x3e317c62full, 0x3a210862eull, 0x3e318c62full,
    0x7c217843full, 0x04217843full, 0x7a390862eull, 0x4631fc631ull, 0x38842108eull, 0x3a3184210ull, 0x452519531ull, 0x7c2108421ull,
    0x46318d771ull, 0x4631cd671ull, 0x3a318c62eull, 0x04217c62full, 0x59358c62eull, 0x45257c62full, 0x3a307062eull, 0x10842109full,
    0x3a318c631ull, 0x11518c631ull, 0x2ab5ac631ull, 0x462a22a31ull, 0x108422a31ull, 0x7c222221full};
constexpr const char *kDrawFontChars = " .0123456789abcdefghijklmnopqrstuvwxyz";
// box / tag colour of class c: draw_palette(c % 8), bytes R, G << 8, B << 16 (a function, so that device code can index the one table)
Y2D_HD inline uint32_t draw_palette(int k)
{
    const uint32_t palette[8] = {0x1e1eff, 0x1eff1e, 0xff1e1e, 0x1effff, 0xff1eff, 0xffff1e, 0x1e80ff, 0xff1e80};
    return palette[k];
}

// a character's glyph; anything outside the font's set is the blank
Y2D_HD inline int draw_glyph_index(char c)
{
    if (c == '.') return 1;
    if (c >= '0' && c <= '9') return 2 + (c - '0');
    if (c >= 'a' && c <= 'z') return 12 + (c - 'a');
    if (c >= 'A' && c <= 'Z') return 12 + (c - 'A');
    return 0;
}

// Everything one drawn record paints, in image coordinates.  Paint order: ring[0], ring[1], the tag rectangle, the glyphs.
struct DrawItem {
    int ring[kDrawThick][4];   // xx0, yy0, xx1, yy1 of border ring t: rows yy0 / yy1 over xx0..xx1, columns xx0 / xx1 over yy0..yy1
    int tag[4];                // the filled rectangle x0, y0, x1, y1 (inclusive, clamped to the image)
    int gx, gy, nchar;         // the text's top-left pixel (may lie outside the image) and its length
    uint32_t box_rgb, text_rgb;
    int ext[4];                // x0, y0, x1, y1 around everything above
    uint8_t text[kDrawMaxText + 1];   // glyph indices
};

// (int)v as the reference compiled for x86-64 has it: NaN and values outside int's range give INT_MIN
Y2D_HD inline int draw_to_int(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN; }
Y2D_HD inline int draw_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The rule both makers share: which records are drawn at all - not prob <= thresh (false for a NaN prob, as in the reference's loop),
// not a negative class (which the reference's best-class loop never yields)
Y2D_HD inline bool draw_is_drawn(const DrawDet &d, float thresh) { return !(d.prob <= thresh || d.cls < 0); }

// Everything of a drawn record's item but its text: corners, rings, colours, tag, gx / gy, ext, for a text of nchar glyphs (it->nchar).
Y2D_HD inline void draw_item_geometry(const DrawDet &d, int width, int height, int nchar, DrawItem *it)
{
    const float hw = d.w * 0.5f, hh = d.h * 0.5f;
    const int x0 = draw_clamp(draw_to_int((d.x - hw) * (float)width), 0, width - 1);
    const int y0 = draw_clamp(draw_to_int((d.y - hh) * (float)height), 0, height - 1);
    const int x1 = draw_clamp(draw_to_int((d.x + hw) * (float)width), 0, width - 1);
    const int y1 = draw_clamp(draw_to_int((d.y + hh) * (float)height), 0, height - 1);
    // the rectangle: corners sorted, then every ring clamped again
    const int rx0 = x0 < x1 ? x0 : x1, rx1 = x0 < x1 ? x1 : x0, ry0 = y0 < y1 ? y0 : y1, ry1 = y0 < y1 ? y1 : y0;
    for (int t = 0; t < kDrawThick; ++t) {
        it->ring[t][0] = draw_clamp(rx0 + t, 0, width - 1);
        it->ring[t][1] = draw_clamp(ry0 + t, 0, height - 1);
        it->ring[t][2] = draw_clamp(rx1 - t, 0, width - 1);
        it->ring[t][3] = draw_clamp(ry1 - t, 0, height - 1);
    }
    it->box_rgb = draw_palette(d.cls % 8);
    const unsigned sum = (it->box_rgb & 255u) + ((it->box_rgb >> 8) & 255u) + (it->box_rgb >> 16);
    it->text_rgb = sum > 382u ? 0u : 0xffffffu;
    it->nchar = nchar;
    const int tw = nchar > 0 ? (nchar * 6 - 1) * kDrawScale : 0, th = kDrawGlyphH;
    const int tx = x0;   // (the unsorted corner)
    int ty = y0 - th - kDrawPad * 2;
    if (ty < 0) ty = y0 + 1;
    it->tag[0] = draw_clamp(tx, 0, width - 1);
    it->tag[1] = draw_clamp(ty, 0, height - 1);
    it->tag[2] = draw_clamp(tx + tw + kDrawPad * 2, 0, width - 1);
    it->tag[3] = draw_clamp(ty + th + kDrawPad * 2, 0, height - 1);
    it->gx = tx + kDrawPad;
    it->gy = ty + kDrawPad;
    for (int k = 0; k < 4; ++k) it->ext[k] = it->tag[k];
    for (int t = 0; t < kDrawThick; ++t)
        for (int k = 0; k < 4; ++k) {
            const int lo = k & 1, hi = 2 + (k & 1);
            if (it->ring[t][k] < it->ext[lo]) it->ext[lo] = it->ring[t][k];
            if (it->ring[t][k] > it->ext[hi]) it->ext[hi] = it->ring[t][k];
        }
}

// ---- the text without snprintf: "%s %.2f" as glyph indices, for the device (k_draw_items) and, through y2h_draw_text, the CPU tests
//
// "%.2f" of a float in integers.  prob = m * 2^e with a 24-bit m, so 100 * m fits 32 bits; below 2^23 e is negative, the value times
// 100 is (100 * m) >> -e with an exact remainder, and printf rounds to nearest, ties to even, on exactly that remainder.

// can the formatter below print it?  (finite and |prob| < 2^23; the loop entry counts drawn records for which this is false)
Y2D_HD inline bool draw_prob_printable(float prob)
{
    uint32_t b;
    memcpy(&b, &prob, 4);
    return ((b >> 23) & 255u) < 127u + 23u;
}
// |prob| * 100 rounded as "%.2f" rounds it
Y2D_HD inline uint32_t draw_prob_hundredths(float prob)
{
    uint32_t b;
    memcpy(&b, &prob, 4);
    const uint32_t eb = (b >> 23) & 255u, frac = b & 0x7fffffu;
    const uint64_t n = 100ull * (eb ? (frac | 0x800000u) : frac);
    const int s = eb ? 150 - (int)eb : 149;   // >= 1 for a printable prob
    if (s > 63) return 0;                       // (n < 2^31: nowhere near half of 2^s)
    const uint64_t q = n >> s, rem = n & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    return (uint32_t)(q + ((rem > half || (rem == half && (q & 1ull))) ? 1u : 0u));
}
// appends the decimal digits of v at out[at...], never past kDrawMaxText glyphs; returns the new length
Y2D_HD inline int draw_put_uint(uint32_t v, uint8_t *out, int at)
{
    char dig[10];
    int nd = 0;
    do { dig[nd++] = (char)(v % 10u); v /= 10u; } while (v);
    while (nd > 0 && at < kDrawMaxText) out[at++] = (uint8_t)(2 + dig[--nd]);
    return at;
}
// The glyph indices of snprintf(char[128], "%s %.2f", label, (double)prob), truncated at 127 as snprintf truncates.  label: glyph
// indices, or NULL for "class<cls>" (cls >= 0).  out [128] is zero behind the text, as DrawItem::text is.  Returns the length, or -1
// (out all zero) where !draw_prob_printable(prob).
Y2D_HD inline int draw_text_glyphs(const uint8_t *label, int label_len, int cls, float prob, uint8_t *out)
{
    for (int i = 0; i <= kDrawMaxText; ++i) out[i] = 0;
    if (!draw_prob_printable(prob)) return -1;
    int at = 0;
    if (label) {
        for (int i = 0; i < label_len && at < kDrawMaxText; ++i) out[at++] = label[i];
    } else {
        const uint8_t word[5] = {12 + 2, 12 + 11, 12 + 0, 12 + 18, 12 + 18};   // c l a s s
        for (int i = 0; i < 5; ++i) out[at++] = word[i];
        at = draw_put_uint((uint32_t)cls, out, at);
    }
    if (at < kDrawMaxText) out[at++] = 0;   // the blank
    uint32_t b;
    memcpy(&b, &prob, 4);
    if ((b >> 31) && at < kDrawMaxText) out[at++] = 0;   // '-' is outside the font
    const uint32_t h = draw_prob_hundredths(prob);
    at = draw_put_uint(h / 100u, out, at);
    if (at < kDrawMaxText) out[at++] = 1;   // '.'
    if (at < kDrawMaxText) out[at++] = (uint8_t)(2 + (h % 100u) / 10u);
    if (at < kDrawMaxText) out[at++] = (uint8_t)(2 + h % 10u);
    return at;
}

// One label of a call's device label table: kDrawLabelStride bytes, [0] its length (0..127; kDrawNoLabel for a null entry), then glyphs
constexpr int kDrawLabelStride = 128;
constexpr uint8_t kDrawNoLabel = 255;
inline void draw_label_entry(const char *label, uint8_t *entry)
{
    memset(entry, 0, (size_t)kDrawLabelStride);
    if (!label) { entry[0] = kDrawNoLabel; return; }
    int n = 0;
    while (n < kDrawMaxText && label[n]) { entry[1 + n] = (uint8_t)draw_glyph_index(label[n]); ++n; }
    entry[0] = (uint8_t)n;
}

// One record -> its item without libc, for records whose prob the formatter prints: false where the record is not drawn OR its prob is
// not printable (*unprintable says which).  label_table: n_labels entries of draw_label_entry, or NULL.
Y2D_HD inline bool draw_item_from_record(const DrawDet &d, int width, int height, float thresh, const uint8_t *label_table, int n_labels,
                                         DrawItem *it, bool *unprintable)
{
    *unprintable = false;
    if (!draw_is_drawn(d, thresh)) return false;
    if (!draw_prob_printable(d.prob)) { *unprintable = true; return false; }
    const uint8_t *e = (label_table && d.cls < n_labels) ? label_table + (size_t)d.cls * kDrawLabelStride : nullptr;
    if (e && e[0] == kDrawNoLabel) e = nullptr;
    const int nchar = draw_text_glyphs(e ? e + 1 : nullptr, e ? (int)e[0] : 0, d.cls, d.prob, it->text);
    draw_item_geometry(d, width, height, nchar, it);
    return true;
}

// One record -> its item; false if the record is not drawn (prob <= thresh; a negative class, which the reference's best-class loop
// never yields).  labels may be NULL; a NULL labels[cls] gives "class<cls>" too (the reference hands it to %s, which is undefined there).
// The text is the host's own snprintf.
inline bool draw_make_item(const DrawDet &d, int width, int height, float thresh, const char *const *labels, int n_labels, DrawItem *it)
{
    if (!draw_is_drawn(d, thresh)) return false;
    char fallback[32];
    const char *label;
    if (labels && d.cls < n_labels && labels[d.cls]) label = labels[d.cls];
    else { snprintf(fallback, sizeof(fallback), "class%d", d.cls); label = fallback; }
    char text[kDrawMaxText + 1];
    snprintf(text, sizeof(text), "%s %.2f", label, (double)d.prob);
    const int nchar = (int)strlen(text);
    memset(it->text, 0, sizeof(it->text));
    for (int i = 0; i < nchar; ++i) it->text[i] = (uint8_t)draw_glyph_index(text[i]);
    draw_item_geometry(d, width, height, nchar, it);
    return true;
}

}  // namespace y2d
