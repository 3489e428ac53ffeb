// draw_list.hpp -- the annotated frame of the reference's camera / video loop as data: what yolo2_draw_detections_rgb24
// (linux_app/src/yolo2_draw.c:276-369) paints for one detection record, worked out on the host as one DrawItem.  Plain C++, no HIP:
// the host restatement (host/y2_host.cpp, y2h::draw_detections_rgb24) paints items one after the other like the reference does, and
// the GPU entries (yolo2_draw.hip) upload them for k_annotate_batch (kernels_draw.hpp), which asks per pixel which item painted last.
// Corner casts and the "%s %.2f" text are made here, by the host's own arithmetic and snprintf, so both are the reference's by
// construction.  The font and the palette are this project's own tables, recovered from what the compiled reference renders
// (tests/golden/make_draw_golden.py renders every glyph; tests/test_draw_host.py compares).
#pragma once
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

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
// box / tag colour of class c: kDrawPalette[c % 8], bytes R, G << 8, B << 16
constexpr uint32_t kDrawPalette[8] = {0x1e1eff, 0x1eff1e, 0xff1e1e, 0x1effff, 0xff1eff, 0xffff1e, 0x1e80ff, 0xff1e80};

// a character's glyph; anything outside the font's set is the blank
inline int draw_glyph_index(char c)
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
inline int draw_to_int(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN; }
inline int draw_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One record -> its item; false if the record is not drawn (prob <= thresh; a negative class, which the reference's best-class loop
// never yields).  labels may be NULL; a NULL labels[cls] gives "class<cls>" too (the reference hands it to %s, which is undefined there).
inline bool draw_make_item(const DrawDet &d, int width, int height, float thresh, const char *const *labels, int n_labels, DrawItem *it)
{
    if (d.prob <= thresh || d.cls < 0) return false;
    char fallback[32];
    const char *label;
    if (labels && d.cls < n_labels && labels[d.cls]) label = labels[d.cls];
    else { snprintf(fallback, sizeof(fallback), "class%d", d.cls); label = fallback; }
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
    it->box_rgb = kDrawPalette[d.cls % 8];
    const unsigned sum = (it->box_rgb & 255u) + ((it->box_rgb >> 8) & 255u) + (it->box_rgb >> 16);
    it->text_rgb = sum > 382u ? 0u : 0xffffffu;
    char text[kDrawMaxText + 1];
    snprintf(text, sizeof(text), "%s %.2f", label, (double)d.prob);
    it->nchar = (int)strlen(text);
    memset(it->text, 0, sizeof(it->text));
    for (int i = 0; i < it->nchar; ++i) it->text[i] = (uint8_t)draw_glyph_index(text[i]);
    const int tw = it->nchar > 0 ? (it->nchar * 6 - 1) * kDrawScale : 0, th = kDrawGlyphH;
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
            int &lo = it->ext[k & 1], &hi = it->ext[2 + (k & 1)];
            if (it->ring[t][k] < lo) lo = it->ring[t][k];
            if (it->ring[t][k] > hi) hi = it->ring[t][k];
        }
    return true;
}

}  // namespace y2d
