// y2_host.hpp -- the repo's own host side of the YOLOv2 path: Darknet .cfg parser, image I/O and
// letterbox, weight-file loading, region layer + box decode + NMS.  Plain C++17, no dependency on
// the oracle and none on the GPU library except in yolov2_detect.cpp.  Each function cites the
// reference behaviour it reproduces (paths relative to the reference repository).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace y2h {

// ---------------------------------------------------------------- cfg (src/core/yolo_net.cpp:218-291)
enum LayerType { CONV = 0, MAXPOOL = 1, REORG = 2, ROUTE = 3, REGION = 4 };  // yolo2_config.h:118-122
struct Layer {
    LayerType type = CONV;
    int c = 0, h = 0, w = 0;              // input
    int out_c = 0, out_h = 0, out_w = 0;  // output
    int n = 0, size = 0, stride = 1, pad = 0;
    bool leaky = false, batch_normalize = false;
    std::vector<int> route_layers;        // absolute indices
    // region
    int classes = 0, coords = 4, num = 0;
    bool softmax = false, background = false;
    std::vector<float> anchors;
};
struct Network {
    int w = 0, h = 0, c = 0;
    std::vector<Layer> layers;
};
Network parse_cfg(const std::string &path);   // throws std::runtime_error

// ---------------------------------------------------------------- images (src/core/yolo_image.cpp)
struct Image {
    int w = 0, h = 0, c = 0;
    std::vector<float> data;  // CHW, [0,1]
    float &at(int x, int y, int k) { return data[(size_t)k * h * w + (size_t)y * w + x]; }
    float at(int x, int y, int k) const { return data[(size_t)k * h * w + (size_t)y * w + x]; }
};
Image make_image(int w, int h, int c);
Image load_pnm(const std::string &path);                 // binary P6 (RGB) / P5 (grey), 8-bit
// the same file as interleaved bytes (what stbi_load hands load_image_stb before its /255.): RGB, grey replicated
struct ImageU8 {
    int w = 0, h = 0;
    std::vector<uint8_t> rgb;   // [h][w][3]
};
ImageU8 load_pnm_u8(const std::string &path);
// The host's own JPEG (baseline, extended-sequential, progressive) and PNG decoders (y2_codec.cpp): the bytes stbi_load(file, 3)
// of the reference's vendored stb_image v2.19 hands load_image_stb (src/core/yolo_image.cpp:167-189), reproduced byte for byte.
ImageU8 decode_jpeg(const uint8_t *data, size_t n);       // throw std::runtime_error
ImageU8 decode_png(const uint8_t *data, size_t n);
ImageU8 decode_image(const uint8_t *data, size_t n, const std::string &name);   // by signature
ImageU8 load_image_u8(const std::string &path);           // JPEG / PNG / binary PNM by signature
Image load_image(const std::string &path);                // load_image_stb(path, 3): + bytes / 255 into CHW floats
void save_ppm(const Image &im, const std::string &path);
Image resize_image(const Image &im, int w, int h);        // yolo_image.cpp:84-126 (two-pass bilinear)
Image letterbox_image(const Image &im, int w, int h);     // yolo_image.cpp:148-165 (grey 0.5 bars)
// A packed YUYV 4:2:2 camera frame (V4L2 'YUYV': bytes Y0 U Y1 V per pixel pair, 2 w bytes per row) -> RGB24 [h][w][3], the
// conversion of the reference's camera loop (yolo2_yuyv_to_rgb24, linux_app/src/yolo2_v4l2.c:328-374): integer BT.601, arithmetic
// shift, clamp to 0..255.  The GPU entries compute the same byte per fetched pixel (csrc/letterbox.hpp, LbYuyv).  False for an odd
// or non-positive width / height (the reference converts pairs over the flat stream and leaves an odd frame's last pixel unwritten).
bool yuyv_to_rgb24(const uint8_t *yuyv, uint8_t *rgb, int w, int h);
// A planar YUV 4:2:0 frame (w h 3 / 2 bytes: the Y plane [h][w], then semi ? NV12's plane [h/2][w/2][2] of U V pairs : I420's U plane
// [h/2][w/2] and V plane [h/2][w/2]) -> RGB24 by the same formula: pixel (x, y) from Y(y, x), U(y >> 1, x >> 1), V(y >> 1, x >> 1), chroma
// replicated.  The library's own extension of the reference's conversion (the reference has no 4:2:0 input); the GPU entries compute
// the same byte per fetched pixel (csrc/letterbox.hpp, LbYuv420).  False for a null pointer or an odd or non-positive width / height.
bool yuv420_to_rgb24(const uint8_t *frame, uint8_t *rgb, int w, int h, bool semi);
// The way out: an RGB24 frame -> NV12 (semi) or I420, w * h * 3 / 2 bytes, the layout above.  Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
// per pixel; U = ((-38 Rs - 74 Gs + 112 Bs + 512) >> 10) + 128 and V = ((112 Rs - 94 Gs - 18 Bs + 512) >> 10) + 128 per 2x2 block from the
// sums of its four pixels.  The library's own definition (the reference has no YUV output; not swscale's); the loop's 4:2:0 painters
// compute the same bytes (csrc/kernels_draw.hpp).  False for a null pointer or an odd or non-positive width / height, nothing written.
bool rgb24_to_yuv420(const uint8_t *rgb, uint8_t *frame, int w, int h, bool semi);
// A packed BGR24 (B G R, w h 3 bytes), RGBA32 (R G B X, w h 4 bytes) or BGRA32 (B G R X) frame -> RGB24: the bytes reordered, the fourth
// byte not read.  fmt: kFrameBgr24 / kFrameRgba32 / kFrameBgra32 below.  The GPU entries pick the same byte per fetched pixel
// (csrc/letterbox.hpp, LbPacked).  False for a null pointer, a non-positive width / height or another fmt.
bool packed_to_rgb24(const uint8_t *src, uint8_t *rgb, int w, int h, int fmt);
void draw_box(Image &im, int x1, int y1, int x2, int y2, int thick, float r, float g, float b);
// The annotated frame of the reference's camera / video loop: yolo2_draw_detections_rgb24 (linux_app/src/yolo2_draw.c:276-369, called
// at linux_app/src/main.c:1079-1091) on records of the library's yolo2_hip_det layout in the YOLO2_DETS_BEST_CLASS form (one per
// detection).  Per record with prob > thresh, in array order: a 2-pixel box in palette[cls % 8], a tag "<label> <prob %.2f>" above
// the box (below its top edge when fewer than 18 rows are free) in the same colour with black or white 5x7 text at scale 2; labels
// may be NULL ("class<N>", also for cls >= n_labels).  Bit-identical to the reference (tests/golden/draw.npz).  Returns the records drawn.
struct DrawRecord {
    int frame, det, cls;
    float prob, x, y, w, h;
};
int draw_detections_rgb24(uint8_t *rgb, int w, int h, const DrawRecord *dets, int n, float thresh, const char *const *labels, int n_labels);
// The streaming CLI's own annotated frame (without --annotate-gpu): the frame's bytes (fmt: RGB24, a packed YUYV frame through
// yuyv_to_rgb24, an NV12 / I420 frame through yuv420_to_rgb24, or a BGR24 / RGBA32 / BGRA32 frame through packed_to_rgb24) as a float image, one draw_box per record in a hue colour of its class, thickness max(1, h * .006).  No labels.
// Throws std::runtime_error for a bad YUYV / 4:2:0 frame.
enum { kFrameRgb24 = 0, kFrameYuyv = 1, kFrameNv12 = 2, kFrameI420 = 3, kFrameBgr24 = 4, kFrameRgba32 = 5, kFrameBgra32 = 6 };
Image plain_box_frame(const uint8_t *bytes, int w, int h, int fmt, const DrawRecord *recs, int n, int classes);
int draw_font(char *chars, uint64_t *words);   // the packed font: 38 characters and their 35-bit glyph words (bit 5 * row + column)
// The annotated frame as the JPEG stream the reference's MJPEG streamer sends (stb_image_write v1.09's stbi_write_jpg_to_func with 3
// components, linux_app/src/yolo2_mjpeg_server.c:221-238), byte for byte (y2_jpeg.cpp; tests/golden/jpeg.npz): baseline, no
// subsampling, quality clamped to 1..100.  Returns the stream's length and stores the bytes below `cap` (out may be NULL if cap is
// 0); -1 for a null frame or a width / height outside 1..65535.  jpg_rgb24_bound: the most bytes a w x h frame can take (0: bad size).
long write_jpg_rgb24(const uint8_t *rgb, int w, int h, int quality, uint8_t *out, size_t cap);
size_t jpg_rgb24_bound(int w, int h);

// ---------------------------------------------------------------- weights (yolo2_model.cpp:158-227)
struct WeightsI16 {
    std::vector<int16_t> weights, bias;      // per-layer file pads stripped
    std::vector<int32_t> weight_q, bias_q, act_q;
};
WeightsI16 load_weights_int16(const std::string &dir, const std::vector<int> &wlen, const std::vector<int> &blen);

// ---------------------------------------------------------------- region + boxes + NMS
struct Box { float x, y, w, h; };
struct Detection {
    Box bbox{};
    float objectness = 0;
    std::vector<float> prob;
    int sort_class = -1;
};
// forward_region_layer (src/core/yolo_region.cpp:123-141): logistic on x,y,obj (double exp),
// softmax over classes with stride w*h reading the RAW input.  in/out: [num][coords+1+classes][h][w]
void region_forward(const Layer &l, const float *in, float *out);
// get_network_boxes -> get_region_detections + correct_region_boxes (yolo_region.cpp:170-236),
// relative = 1.  Returns w*h*num detections, objectness 0 for those at or below thresh.
std::vector<Detection> region_boxes(const Layer &l, const float *out, int im_w, int im_h, int net_w, int net_h, float thresh);
// do_nms_sort (src/core/yolo_post.cpp:54-85): drops objectness==0, per-class sort + IoU suppression.
// Returns the number of detections kept in front.
int nms_sort(std::vector<Detection> &dets, int classes, float thresh);
float box_iou(const Box &a, const Box &b);

Layer yolo2_region_layer();

// The tail of the path for a whole batch (at thousands of frames/s a single
// thread of region + NMS is the bottleneck): int16 region tensors [batch][425][13][13] with final
// Q -> dequantise (yolo2_model.cpp:415-417), region_forward, region_boxes, nms_sort per frame,
// frames spread over `threads` host threads.  Per frame exactly the single-frame functions above,
// so the results are identical to calling them in a loop.  Returns, per frame, the detections kept
// in front by nms_sort (all w*h*num of them if nms <= 0).
std::vector<std::vector<Detection>> postprocess_batch(const int16_t *region, int batch, int final_q, const int *im_w,
                                                      const int *im_h, float thresh, float nms, int threads);

// ---------------------------------------------------------------- the camera loop's tail
// The reference's camera / video loop (linux_app/src/main.c:1013-1026, :1184-1197) and its single-image mode (:827-858) run
// linux_app/src/yolo2_postprocess.c, not the src/core tail above, and the two round differently.  These restate it bit for bit
// (tests/golden/apptail.npz):
// yolo2_forward_region_layer (:106-135): sigmoid 1.0f / (1.0f + expf(-x)) with x > 10 -> 1 and x < -10 -> 0 on x, y, objectness;
// softmax with expf, a float sum in class order and *= 1.0f / sum (1 / n for a sum <= 0), in place over the raw class entries.
void app_region_forward(const Layer &l, const float *in, float *out);
// yolo2_get_region_detections (:140-196) + correct_region_boxes (:77-101, all float), relative = 1.  Returns ONLY the candidates
// (objectness > thresh), cells in raster order and anchors inner; there are no zeroed slots behind them.
std::vector<Detection> app_region_detections(const Layer &l, const float *out, int im_w, int im_h, int net_w, int net_h, float thresh);
// yolo2_do_nms_sort (:248-284) with the app's box_iou (:199-226: fminf / fmaxf, * 0.5f, 0 for an overlap or a union <= 0).  The app
// runs it at every threshold, 0 included.  Returns the number of detections kept in front.
int app_nms_sort(std::vector<Detection> &dets, int classes, float thresh);
float app_box_iou(const Box &a, const Box &b);
// postprocess_batch with the three functions above: per frame exactly the single-frame calls (app_nms_sort whenever a frame has a
// candidate, as main.c:856-858 does).
std::vector<std::vector<Detection>> postprocess_batch_app(const int16_t *region, int batch, int final_q, const int *im_w,
                                                          const int *im_h, float thresh, float nms, int threads);

std::vector<std::string> load_names(const std::string &path);

}  // namespace y2h
