// pix_formats.hpp -- the pixel formats of the _pix entries, stated once for the kernels, the library's tables and the CLIs (plain C++,
// no HIP: host/ includes it as it includes bayer_def.hpp).  A new format is a row of Y2_PIX_FORMATS, its YOLO2_PIX_* constant in
// include/yolo2_hip.h and, unless it reads through an existing fetch, a row of Y2_PIX_KINDS and the fetch struct in letterbox.hpp.
#pragma once
#include <cstddef>

// The kinds: one per pixel fetch (letterbox.hpp), i.e. per set of kernels.  X(kind, short name, LB, I8, F16, fetch type), in the order
// of Y2PixKind.  The kernels of a kind are k_letterbox_<short>[_batch], k_i8_front_<short> and k_conv0_pool_mfma_<short>; the three
// middle columns say where each is written:
//   GEN   generated from this row (kernels_pix.hpp, kernels_i8_front_pix.hpp, kernels_f16_pix.hpp)
//   HAS   written out in kernels_pre.hpp / kernels_f16.hpp, which stay as they are
//   TPL   (I8) launched as k_i8_front_pix<fetch> itself, reported under the short name
//   NONE  (F16) the fp16 passes have no layer-0 step from bytes for this kind
// (the Bayer kinds in the order of their ch, kLbChBayer + rx + 2 * ry)
#define Y2_PIX_KINDS(X)                                          \
    X(BYTES,      u8,         HAS, TPL, HAS,  LbInterleaved)     \
    X(YUYV,       yuyv,       GEN, TPL, HAS,  LbYuyv)            \
    X(NV12,       nv12,       GEN, GEN, GEN,  LbYuv420<true>)    \
    X(I420,       i420,       GEN, GEN, GEN,  LbYuv420<false>)   \
    X(BGR24,      bgr24,      GEN, GEN, GEN,  LbPacked<3, true>) \
    X(RGBA32,     rgba32,     GEN, GEN, GEN,  LbPacked<4, false>) \
    X(BGRA32,     bgra32,     GEN, GEN, GEN,  LbPacked<4, true>) \
    X(BAYER_RGGB, bayer_rggb, GEN, GEN, NONE, LbBayer<0, 0>)     \
    X(BAYER_GRBG, bayer_grbg, GEN, GEN, NONE, LbBayer<1, 0>)     \
    X(BAYER_GBRG, bayer_gbrg, GEN, GEN, NONE, LbBayer<0, 1>)     \
    X(BAYER_BGGR, bayer_bggr, GEN, GEN, NONE, LbBayer<1, 1>)

// The formats, in the order of include/yolo2_hip.h.  X(ID, fourcc, kind, ch, bits, even_w, even_h, align, min_side, cli, alias, frame, msg):
//   ID, fourcc        YOLO2_PIX_<ID> and its value; the library's name for the format is "<ID>"
//   ch                what LetterboxArgs::ch / AnnoFrame::ch carry: bytes per pixel for interleaved bytes (1, 3) and YUYV (2); for the planar
//                     4:2:0 formats, which have no whole number of bytes per pixel, for packed BGR24 / RGBA32 / BGRA32, whose byte counts
//                     3 and 4 would not tell them from RGB24, and for the four raw Bayer patterns (1 byte per pixel, as GREY8) a code that
//                     only their own fetch looks at
//   bits              per pixel: a frame is w * h * bits / 8 bytes
//   even_w / even_h   the parity rule; align: the address alignment the single-image entries ask for (4: the fetch loads dwords)
//   min_side          the least width and height (a Bayer frame has a whole 2 x 2 block: the mirror needs a second row and column)
//   cli, alias        --video-pix-fmt's canonical spelling and its other one (nullptr: none; GREY8 is not a video format)
//   frame             y2h::plain_box_frame's code (host/y2_host.hpp; expanded only where that header is included)
//   msg               the format's part of the "unknown pixel format" message, with what follows it in the sentence (", ", " or ", "; "): the
//                     text is pinned byte for byte, so the fragments are kept by hand - a new last row rewrites its neighbour's ending
#define Y2_PIX_FORMATS(X)                                                                                                                              \
    X(GREY8,       1,          BYTES,      1,  8,  false, false, 1, 1, nullptr,       nullptr, -1,                    "YOLO2_PIX_GREY8, ")           \
    X(RGB24,       3,          BYTES,      3,  24, false, false, 1, 1, "rgb24",       nullptr, y2h::kFrameRgb24,      "YOLO2_PIX_RGB24, ")           \
    X(YUYV,        0x56595559, YUYV,       2,  16, true,  false, 4, 1, "yuyv422",     "yuyv",  y2h::kFrameYuyv,       "YOLO2_PIX_YUYV, ")            \
    X(NV12,        0x3231564E, NV12,       12, 12, true,  true,  1, 1, "nv12",        nullptr, y2h::kFrameNv12,       "YOLO2_PIX_NV12, ")            \
    X(I420,        0x32315559, I420,       13, 12, true,  true,  1, 1, "yuv420p",     "i420",  y2h::kFrameI420,       "YOLO2_PIX_I420, ")            \
    X(BGR24,       0x33524742, BGR24,      24, 24, false, false, 1, 1, "bgr24",       nullptr, y2h::kFrameBgr24,      "YOLO2_PIX_BGR24, ")           \
    X(RGBA32,      0x34324241, RGBA32,     32, 32, false, false, 4, 1, "rgba",        "rgb0",  y2h::kFrameRgba32,     "YOLO2_PIX_RGBA32 or ")        \
    X(BGRA32,      0x34325241, BGRA32,     33, 32, false, false, 4, 1, "bgra",        "bgr0",  y2h::kFrameBgra32,     "YOLO2_PIX_BGRA32; ")          \
    X(BAYER_RGGB8, 0x42474752, BAYER_RGGB, 80, 8,  false, false, 1, 2, "bayer_rggb8", nullptr, y2h::kFrameBayer + 0,  "YOLO2_PIX_BAYER_RGGB8, ")     \
    X(BAYER_BGGR8, 0x31384142, BAYER_BGGR, 83, 8,  false, false, 1, 2, "bayer_bggr8", nullptr, y2h::kFrameBayer + 3,  "_BGGR8, ")                    \
    X(BAYER_GRBG8, 0x47425247, BAYER_GRBG, 81, 8,  false, false, 1, 2, "bayer_grbg8", nullptr, y2h::kFrameBayer + 1,  "_GRBG8 or ")                  \
    X(BAYER_GBRG8, 0x47524247, BAYER_GBRG, 82, 8,  false, false, 1, 2, "bayer_gbrg8", nullptr, y2h::kFrameBayer + 2,  "_GBRG8")

// which kernels read a frame (the letterbox, layer-0, int8-front and painter instantiations)
#define Y2_PIX_ROW(KIND, SHORT, LB, I8, F16, ...) Y2_KIND_##KIND,
enum Y2PixKind { Y2_PIX_KINDS(Y2_PIX_ROW) Y2_KIND_COUNT };
#undef Y2_PIX_ROW

namespace y2pix {

#define Y2_PIX_ROW(ID, FOURCC, ...) ID = FOURCC,
enum Fourcc : int { Y2_PIX_FORMATS(Y2_PIX_ROW) };   // y2pix::NV12 == YOLO2_PIX_NV12
#undef Y2_PIX_ROW

struct Format {
    int pixfmt;
    const char *name;
    Y2PixKind kind;
    int ch, bits;
    bool even_w, even_h;
    unsigned align;
    int min_side;
    const char *cli, *alias;
    constexpr size_t frame_bytes(int w, int h) const { return (size_t)w * h * bits / 8; }
};
#define Y2_PIX_ROW(ID, FOURCC, KIND, CH, BITS, EVEN_W, EVEN_H, ALIGN, MIN_SIDE, CLI, ALIAS, FRAME, MSG) \
    {FOURCC, #ID, Y2_KIND_##KIND, CH, BITS, EVEN_W, EVEN_H, ALIGN, MIN_SIDE, CLI, ALIAS},
inline constexpr Format kFormats[] = {Y2_PIX_FORMATS(Y2_PIX_ROW)};
#undef Y2_PIX_ROW

constexpr const Format *by_fourcc(int pixfmt)
{
    for (const Format &f : kFormats)
        if (f.pixfmt == pixfmt) return &f;
    return nullptr;
}
constexpr int ch_of(int pixfmt) { return by_fourcc(pixfmt)->ch; }

#ifdef YOLO2_HIP_H   // (include/yolo2_hip.h was included first: the rows are the public constants)
#define Y2_PIX_ROW(ID, FOURCC, ...) static_assert((int)ID == (int)YOLO2_PIX_##ID, "pix_formats.hpp: " #ID " is not YOLO2_PIX_" #ID);
Y2_PIX_FORMATS(Y2_PIX_ROW)
#undef Y2_PIX_ROW
#endif

}  // namespace y2pix
