// y2_host_capi.cpp -- extern "C" doorway into the host logic for the Python tests
// (libyolo2_host.so).  No GPU involved.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>

#include "../csrc/draw_list.hpp"
#include "y2_host.hpp"

using namespace y2h;

static thread_local std::string g_err;

extern "C" {
const char *y2h_last_error() { return g_err.c_str(); }

// desc[i*12 + {type,c,h,w,out_c,out_h,out_w,n,size,stride,pad,leaky}]; returns layer count or -1
int y2h_parse_cfg(const char *path, int *net_whc, int *desc, int max_layers, float *anchors10, int *region_params)
{
    try {
        Network n = parse_cfg(path);
        net_whc[0] = n.w; net_whc[1] = n.h; net_whc[2] = n.c;
        int i = 0;
        for (const Layer &l : n.layers) {
            if (i >= max_layers) break;
            int v[12] = {l.type, l.c, l.h, l.w, l.out_c, l.out_h, l.out_w, l.n, l.size, l.stride, l.pad, (int)l.leaky};
            memcpy(desc + i * 12, v, sizeof(v));
            if (l.type == REGION) {
                for (size_t k = 0; k < l.anchors.size() && k < 10; ++k) anchors10[k] = l.anchors[k];
                region_params[0] = l.classes; region_params[1] = l.coords; region_params[2] = l.num; region_params[3] = l.softmax;
            }
            ++i;
        }
        return (int)n.layers.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

void y2h_letterbox(const float *chw, int w, int h, int c, int nw, int nh, float *out)
{
    Image im = make_image(w, h, c);
    memcpy(im.data.data(), chw, sizeof(float) * (size_t)w * h * c);
    Image o = letterbox_image(im, nw, nh);
    memcpy(out, o.data.data(), sizeof(float) * (size_t)nw * nh * c);
}

void y2h_region_forward(const float *in, float *out) { region_forward(yolo2_region_layer(), in, out); }

// out rows: [x, y, w, h, objectness, prob[80]] for the `kept` detections in front; returns kept
int y2h_boxes_nms(const float *region_proc, int im_w, int im_h, float thresh, float nms, float *out, int max_rows)
{
    const Layer l = yolo2_region_layer();
    std::vector<Detection> d = region_boxes(l, region_proc, im_w, im_h, 416, 416, thresh);
    int total = (int)d.size();
    if (nms > 0) total = nms_sort(d, l.classes, nms);
    int rows = total < max_rows ? total : max_rows;
    for (int i = 0; i < rows; ++i) {
        float *r = out + (size_t)i * 85;
        r[0] = d[i].bbox.x; r[1] = d[i].bbox.y; r[2] = d[i].bbox.w; r[3] = d[i].bbox.h; r[4] = d[i].objectness;
        memcpy(r + 5, d[i].prob.data(), sizeof(float) * 80);
    }
    return total;
}

// rows_out: [batch][max_rows][85] = {x, y, w, h, objectness, prob[80]}; totals[f] = detections kept for frame f
int y2h_postprocess_batch(const int16_t *region, int batch, int final_q, const int *im_w, const int *im_h, float thresh,
                          float nms, int threads, float *rows_out, int max_rows, int *totals)
{
    try {
        auto all = postprocess_batch(region, batch, final_q, im_w, im_h, thresh, nms, threads);
        for (int f = 0; f < batch; ++f) {
            const auto &d = all[(size_t)f];
            totals[f] = (int)d.size();
            const int rows = std::min((int)d.size(), max_rows);
            for (int i = 0; i < rows; ++i) {
                float *r = rows_out + ((size_t)f * max_rows + i) * 85;
                r[0] = d[i].bbox.x; r[1] = d[i].bbox.y; r[2] = d[i].bbox.w; r[3] = d[i].bbox.h; r[4] = d[i].objectness;
                memcpy(r + 5, d[i].prob.data(), sizeof(float) * 80);
            }
        }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// the camera loop's tail (linux_app/src/yolo2_postprocess.c): same layout as y2h_postprocess_batch
int y2h_postprocess_app_batch(const int16_t *region, int batch, int final_q, const int *im_w, const int *im_h, float thresh,
                              float nms, int threads, float *rows_out, int max_rows, int *totals)
{
    try {
        auto all = postprocess_batch_app(region, batch, final_q, im_w, im_h, thresh, nms, threads);
        for (int f = 0; f < batch; ++f) {
            const auto &d = all[(size_t)f];
            totals[f] = (int)d.size();
            const int rows = std::min((int)d.size(), max_rows);
            for (int i = 0; i < rows; ++i) {
                float *r = rows_out + ((size_t)f * max_rows + i) * 85;
                r[0] = d[i].bbox.x; r[1] = d[i].bbox.y; r[2] = d[i].bbox.w; r[3] = d[i].bbox.h; r[4] = d[i].objectness;
                memcpy(r + 5, d[i].prob.data(), sizeof(float) * 80);
            }
        }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

void y2h_app_region_forward(const float *raw, float *proc) { app_region_forward(yolo2_region_layer(), raw, proc); }

int y2h_load_pnm(const char *path, int *whc, float *out, long capacity)
{
    try {
        Image im = load_pnm(path);
        whc[0] = im.w; whc[1] = im.h; whc[2] = im.c;
        if ((long)im.data.size() > capacity) return -2;
        memcpy(out, im.data.data(), sizeof(float) * im.data.size());
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// yuyv_to_rgb24: 0, or -1 (y2h_last_error) for a null pointer, a non-positive size or an odd width
int y2h_yuyv_to_rgb24(const uint8_t *yuyv, uint8_t *rgb, int w, int h)
{
    if (yuyv_to_rgb24(yuyv, rgb, w, h)) return 0;
    g_err = "yuyv_to_rgb24: bad frame " + std::to_string(w) + "x" + std::to_string(h) + " (YUYV frames have an even width)";
    return -1;
}

// draw_detections_rgb24: dets are yolo2_hip_det records; returns the records drawn, or -1 (y2h_last_error) for a null frame or a
// non-positive size
int y2h_draw_detections_rgb24(uint8_t *rgb, int w, int h, const void *dets, int n, float thresh, const char *const *labels, int n_labels)
{
    if (!rgb || w <= 0 || h <= 0 || (n > 0 && !dets)) {
        g_err = "draw_detections_rgb24: null buffer or bad frame " + std::to_string(w) + "x" + std::to_string(h);
        return -1;
    }
    return draw_detections_rgb24(rgb, w, h, static_cast<const DrawRecord *>(dets), n, thresh, labels, n_labels);
}

// yuv420_to_rgb24 (semi: NV12, otherwise I420): 0, or -1 (y2h_last_error) for a null pointer or an odd or non-positive width / height
int y2h_yuv420_to_rgb24(const uint8_t *frame, uint8_t *rgb, int w, int h, int semi)
{
    if (yuv420_to_rgb24(frame, rgb, w, h, semi != 0)) return 0;
    g_err = "yuv420_to_rgb24: bad frame " + std::to_string(w) + "x" + std::to_string(h) + " (NV12 / I420 frames have an even width and an even height)";
    return -1;
}

// rgb24_to_yuv420 (semi_planar: NV12, otherwise I420; out: w * h * 3 / 2 bytes): 0, or -1 (y2h_last_error) with out untouched for a null
// pointer or an odd or non-positive width / height
int y2h_rgb24_to_yuv420(const uint8_t *rgb, int w, int h, int semi_planar, uint8_t *out)
{
    if (rgb24_to_yuv420(rgb, out, w, h, semi_planar != 0)) return 0;
    g_err = "rgb24_to_yuv420: null pointer or bad frame " + std::to_string(w) + "x" + std::to_string(h) + " (NV12 / I420 frames have an even width and an even height)";
    return -1;
}

// packed_to_rgb24; pixfmt: the YOLO2_PIX_* fourcc of BGR24 ('BGR3'), RGBA32 ('AB24') or BGRA32 ('AR24').  0, or -1 (y2h_last_error) for a
// null pointer, a non-positive width / height or another pixfmt
int y2h_packed_to_rgb24(const uint8_t *src, int w, int h, int pixfmt, uint8_t *rgb)
{
    const int fmt = pixfmt == 0x33524742 ? kFrameBgr24 : pixfmt == 0x34324241 ? kFrameRgba32 : pixfmt == 0x34325241 ? kFrameBgra32 : -1;
    if (fmt < 0) {
        char hex[16];
        std::snprintf(hex, sizeof(hex), "0x%x", (unsigned)pixfmt);
        g_err = std::string("packed_to_rgb24: unknown pixel format ") + hex + " (BGR24, RGBA32 or BGRA32)";
        return -1;
    }
    if (packed_to_rgb24(src, rgb, w, h, fmt)) return 0;
    g_err = "packed_to_rgb24: null pointer or bad frame size " + std::to_string(w) + "x" + std::to_string(h);
    return -1;
}

// plain_box_frame, the CLI writer's own frame, for tools/annotate_report.py to time; returns the sum of the image, or -1
// (y2h_last_error) for a bad frame; yuyv: 0 RGB24, 1 YUYV, 2 NV12, 3 I420, 4 BGR24, 5 RGBA32, 6 BGRA32
double y2h_plain_box_frame(const uint8_t *bytes, int w, int h, int yuyv, const void *dets, int n, int classes)
{
    try {
        const Image im = plain_box_frame(bytes, w, h, yuyv, static_cast<const DrawRecord *>(dets), n, classes);
        double sum = 0;
        for (float v : im.data) sum += v;
        return sum;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

int y2h_draw_font(char *chars, uint64_t *words) { return draw_font(chars, words); }

// The shared formatter of csrc/draw_list.hpp (what k_draw_items runs on the device): the glyph indices of
// snprintf(char[128], "%s %.2f", label, prob); label NULL: "class<cls>".  glyphs [128], zero behind the text.  Returns the length, or
// -1 for a prob the formatter does not print (not finite, or 2^23 and more).
int y2h_draw_text(const char *label, int cls, float prob, uint8_t *glyphs)
{
    uint8_t entry[y2d::kDrawLabelStride];
    y2d::draw_label_entry(label, entry);
    return y2d::draw_text_glyphs(label ? entry + 1 : nullptr, label ? (int)entry[0] : 0, cls, prob, glyphs);
}
// One yolo2_hip_det record -> its DrawItem (y2h_draw_item_size() bytes at `item`), by the device's route: a label table made of
// `labels`, then y2d::draw_item_from_record.  1: drawn; 0: not drawn (item untouched); -1: it would be drawn but its prob is not printable.
size_t y2h_draw_item_size() { return sizeof(y2d::DrawItem); }
int y2h_draw_item(const void *det, int w, int h, float thresh, const char *const *labels, int n_labels, void *item)
{
    y2d::DrawDet d;
    memcpy(&d, det, sizeof(d));
    std::string table((size_t)std::max(n_labels, 0) * y2d::kDrawLabelStride, '\0');
    for (int i = 0; labels && i < n_labels; ++i) y2d::draw_label_entry(labels[i], reinterpret_cast<uint8_t *>(&table[0]) + (size_t)i * y2d::kDrawLabelStride);
    y2d::DrawItem it;
    memset(&it, 0, sizeof(it));
    bool unprintable = false;
    const bool drawn = y2d::draw_item_from_record(d, w, h, thresh, labels ? reinterpret_cast<const uint8_t *>(table.data()) : nullptr, n_labels, &it, &unprintable);
    if (drawn) memcpy(item, &it, sizeof(it));
    return drawn ? 1 : (unprintable ? -1 : 0);
}

// write_jpg_rgb24 (y2_jpeg.cpp): returns the stream's length (bytes below cap are stored), or -1 (y2h_last_error)
long y2h_write_jpg_rgb24(const uint8_t *rgb, int w, int h, int quality, uint8_t *out, size_t cap)
{
    const long n = write_jpg_rgb24(rgb, w, h, quality, out, cap);
    if (n < 0) g_err = "write_jpg_rgb24: null buffer or bad frame " + std::to_string(w) + "x" + std::to_string(h) + " (1..65535)";
    return n;
}
size_t y2h_jpg_rgb24_bound(int w, int h) { return jpg_rgb24_bound(w, h); }

// decode_image (y2_codec.cpp): JPEG / PNG bytes -> RGB bytes [h][w][3]; returns w*h*3, or -1 (y2h_last_error) / -2 (capacity)
long y2h_decode_image(const unsigned char *data, long n, int *w, int *h, unsigned char *rgb, long cap)
{
    try {
        const ImageU8 im = decode_image(data, (size_t)n, "<memory>");
        *w = im.w; *h = im.h;
        if ((long)im.rgb.size() > cap) return -2;
        memcpy(rgb, im.rgb.data(), im.rgb.size());
        return (long)im.rgb.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
}
