// letterbox.hpp -- kernels_pre.hpp's letterbox arithmetic for k_conv0_pool_mfma_u8 (kernels_f16.hpp), which builds layer 0's input
// patches from image bytes.  kernels_pre.hpp defines its kernels in the header, so only one translation unit (yolo2_hip.hip) may
// include it, and it is one of the int16 device sources bench.py hashes against the committed traffic measurement: it stays as it
// is.  This header restates its two structs token for token (tests/test_images_f16_abi.py compares them) and its lb_part / lb_value
// with the byte -> v / 255 step as a parameter, so that the fused kernel can take it from a table in LDS.  Every float operation
// is lb_part / lb_value's, in their order: the values are bit-identical (tests/test_gpu_images_f16.py).
// The pixel fetch is a parameter too: LbInterleaved reads kernels_pre.hpp's 1 or 3 interleaved byte channels, LbYuyv turns a packed
// YUYV 4:2:2 pixel into the R, G or B byte first (kernels_pix.hpp, k_conv0_pool_mfma_yuyv), LbYuv420 does the same for the planar
// 4:2:0 frames of video decoders, NV12 and I420 (kernels_pix.hpp, kernels_f16_pix.hpp), LbPacked picks the R, G or B byte of a packed
// BGR24 / RGBA32 / BGRA32 pixel, the frames OpenCV, GUI toolkits and screen capture hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace y2 {

// (kernels_pix.hpp sets Y2_LETTERBOX_STRUCTS_FROM_PRE: in the one translation unit that includes kernels_pre.hpp the two structs
//  are kernels_pre.hpp's own)
#ifndef Y2_LETTERBOX_STRUCTS_FROM_PRE
struct LetterboxArgs {
    int w, h, ch;          // source image: w x h, ch interleaved byte channels (1 or 3)
    int net_w, net_h;      // canvas (416 x 416)
    int new_w, new_h;      // fitted size
    int off_x, off_y;      // where the fitted image sits on the canvas
    float w_scale, h_scale;
};
#endif

// byte -> v / 255.f as load_image_stb computes it
struct LbDiv255 {
    __device__ float operator()(uint8_t v) const { return __fdiv_rn((float)v, 255.f); }
};
// the same values from a 256-entry table of LbDiv255's results (k_conv0_pool_mfma_u8 keeps it in LDS): same bits, no division
struct LbTable {
    const float *t;
    __device__ float operator()(uint8_t v) const { return t[v]; }
};

// The pixel fetch, a type parameter of lb_part_q: which bytes of image row r are byte k of pixel x.
// kernels_pre.hpp's: a.ch interleaved byte channels, a grey image gives its one channel three times (lb_part_q's own lines)
struct LbInterleaved {};
// Packed YUYV 4:2:2 (V4L2 'YUYV', a.ch == 2 bytes per pixel, a.w even): pixels 2p and 2p + 1 are the bytes Y0 U Y1 V at 4p, and
// the byte is the reference camera loop's conversion (yolo2_yuyv_to_rgb24, linux_app/src/yolo2_v4l2.c:328-374): integer BT.601
// with an arithmetic shift and a clamp to 0..255.  The pair is one aligned dword (rows are 2 a.w bytes, the image starts on a
// 4-byte boundary), loaded once per pixel.
struct LbYuyv {
    const uint32_t *row;
    int cu, cv;   // channel k's U and V coefficients
    __device__ LbYuyv(const uint8_t *__restrict__ img, const LetterboxArgs &a, int r, int k)
        : row(reinterpret_cast<const uint32_t *>(img + ((size_t)r * a.w) * 2)), cu(k == 0 ? 0 : (k == 1 ? -100 : 516)),
          cv(k == 0 ? 409 : (k == 1 ? -208 : 0)) {}
    __device__ uint8_t operator()(int x) const
    {
        const uint32_t p = row[x >> 1];
        const int c = (int)((p >> ((x & 1) * 16)) & 255u) - 16, d = (int)((p >> 8) & 255u) - 128, e = (int)(p >> 24) - 128;
        return (uint8_t)min(max((298 * c + cu * d + cv * e + 128) >> 8, 0), 255);
    }
};

// Planar YUV 4:2:0: a full-resolution Y plane [a.h][a.w], then the chroma of every 2 x 2 block of pixels - SEMI (NV12): one plane
// [a.h / 2][a.w / 2] of interleaved U V pairs; otherwise (I420 = yuv420p): a U plane [a.h / 2][a.w / 2], then a V plane of the same shape.
// a.w and a.h are even.  Pixel (x, r) has Y(r, x) and the chroma of (r >> 1, x >> 1), replicated, not interpolated, and its byte is
// LbYuyv's conversion of those three: the frame is the YUYV frame whose row r is Y0 U Y1 V from luma row r and chroma row r >> 1.
// The plane addresses follow from a.w and a.h alone (a.ch is a format code here, not a byte count, and is not read).  All loads are
// byte loads: an I420 chroma row is a.w / 2 bytes and starts anywhere, and the single-image entries take a frame at any address, so
// an NV12 pair is not known to sit on an even address either.
constexpr int kLbChNv12 = 12, kLbChI420 = 13;   // LetterboxArgs::ch / AnnoFrame::ch of the two formats
template <bool SEMI>
struct LbYuv420 {
    const uint8_t *y, *u, *v;   // luma row r; chroma row r >> 1 (SEMI: v = u + 1, pairs two bytes apart)
    int cu, cv;
    __device__ LbYuv420(const uint8_t *__restrict__ img, const LetterboxArgs &a, int r, int k)
        : y(img + (size_t)r * a.w), u(img + (size_t)a.w * a.h + (size_t)(r >> 1) * (SEMI ? a.w : a.w >> 1)),
          v(u + (SEMI ? (size_t)1 : ((size_t)(a.w >> 1) * (a.h >> 1)))), cu(k == 0 ? 0 : (k == 1 ? -100 : 516)),
          cv(k == 0 ? 409 : (k == 1 ? -208 : 0)) {}
    __device__ uint8_t operator()(int x) const
    {
        const int xc = SEMI ? (x & ~1) : (x >> 1);
        const int c = (int)y[x] - 16, d = (int)u[xc] - 128, e = (int)v[xc] - 128;
        return (uint8_t)min(max((298 * c + cu * d + cv * e + 128) >> 8, 0), 255);
    }
};

// Packed RGB in another byte order or with a fourth byte: BPP bytes per pixel, rows of a.w * BPP bytes; byte k (0 R, 1 G, 2 B) of pixel
// x is row[x * BPP + (SWAP ? 2 - k : k)].  BPP 3, SWAP: BGR24 (V4L2 'BGR3', OpenCV's), byte loads, any address.  BPP 4: RGBA32 ('AB24':
// R G B X) and, SWAP, BGRA32 ('AR24': B G R X); the pixel is one aligned dword (rows are 4 a.w bytes, the image starts on a 4-byte
// boundary) and the fourth byte is shifted past, never into a result.  The byte is the source's own: everything after the fetch sees
// what LbInterleaved would on the RGB24 frame with the bytes reordered.  (a.ch is a format code here, not a byte count, and is not read)
constexpr int kLbChBgr24 = 24, kLbChRgba32 = 32, kLbChBgra32 = 33;   // LetterboxArgs::ch / AnnoFrame::ch of the three formats
template <int BPP, bool SWAP>
struct LbPacked {
    static_assert(BPP == 3 || BPP == 4, "three packed bytes, or three and a fourth that is not used");
    const uint8_t *row;   // row r, at channel k's byte (BPP 3) / at the pixel (BPP 4)
    int shift;            // BPP 4: where channel k's byte sits in the pixel's dword
    __device__ LbPacked(const uint8_t *__restrict__ img, const LetterboxArgs &a, int r, int k)
        : row(img + ((size_t)r * a.w) * BPP + (BPP == 3 ? (SWAP ? 2 - k : k) : 0)), shift(8 * (SWAP ? 2 - k : k)) {}
    __device__ uint8_t operator()(int x) const
    {
        if constexpr (BPP == 4) return (uint8_t)(reinterpret_cast<const uint32_t *>(row)[x] >> shift);
        else return row[(size_t)x * 3];
    }
};

// a fetch that converts: lb_part_q runs its operations on the fetch's bytes instead of on interleaved channels
template <class F> struct LbConverts : std::false_type {};
template <> struct LbConverts<LbYuyv> : std::true_type {};
template <bool SEMI> struct LbConverts<LbYuv420<SEMI>> : std::true_type {};
template <int BPP, bool SWAP> struct LbConverts<LbPacked<BPP, SWAP>> : std::true_type {};

// kernels_pre.hpp's lb_part: the horizontally interpolated value part(c, r, k) of resize_image's first pass
template <class Q = LbDiv255, class F = LbInterleaved>
__device__ inline float lb_part_q(const uint8_t *__restrict__ img, const LetterboxArgs &a, int c, int r, int k, Q q = Q())
{
    if constexpr (LbConverts<F>::value) {   // the same operations on the converted bytes
        const F px(img, a, r, k);
        if (c == a.new_w - 1 || a.w == 1) return q(px(a.w - 1));
        const float sx = __fmul_rn((float)c, a.w_scale);
        const int ix = (int)sx;
        const float dx = __fsub_rn(sx, (float)ix);
        const float p0 = q(px(min(ix, a.w - 1)));
        const float p1 = q(px(min(ix + 1, a.w - 1)));
        return __fadd_rn(__fmul_rn(__fsub_rn(1.f, dx), p0), __fmul_rn(dx, p1));
    } else {
        const int kk = a.ch == 3 ? k : 0;
        const uint8_t *row = img + ((size_t)r * a.w) * a.ch + kk;
        if (c == a.new_w - 1 || a.w == 1) return q(row[(size_t)(a.w - 1) * a.ch]);
        const float sx = __fmul_rn((float)c, a.w_scale);
        const int ix = (int)sx;
        const float dx = __fsub_rn(sx, (float)ix);
        const float p0 = q(row[(size_t)min(ix, a.w - 1) * a.ch]);
        const float p1 = q(row[(size_t)min(ix + 1, a.w - 1) * a.ch]);   // (clamp: memory safety only)
        return __fadd_rn(__fmul_rn(__fsub_rn(1.f, dx), p0), __fmul_rn(dx, p1));
    }
}

// kernels_pre.hpp's lb_value for canvas element (k, y, x): 0.5 outside the fitted image, resize_image's second pass inside it
template <class Q = LbDiv255, class F = LbInterleaved>
__device__ inline float lb_value_at(const uint8_t *__restrict__ img, const LetterboxArgs &a, int k, int y, int x, Q q = Q())
{
    const int c = x - a.off_x, r = y - a.off_y;
    float v = .5f;
    if (c >= 0 && c < a.new_w && r >= 0 && r < a.new_h) {
        const float sy = __fmul_rn((float)r, a.h_scale);
        const int iy = (int)sy;
        const float dy = __fsub_rn(sy, (float)iy);
        v = __fmul_rn(__fsub_rn(1.f, dy), lb_part_q<Q, F>(img, a, c, min(iy, a.h - 1), k, q));
        if (!(r == a.new_h - 1 || a.h == 1)) v = __fadd_rn(v, __fmul_rn(dy, lb_part_q<Q, F>(img, a, c, min(iy + 1, a.h - 1), k, q)));
    }
    return v;
}

// one frame of a chunk's staging buffer: where the image's bytes start (relative to the buffer) and its geometry
#ifndef Y2_LETTERBOX_STRUCTS_FROM_PRE
struct LetterboxItem {
    unsigned long long off;
    LetterboxArgs a;
};
#endif

}  // namespace y2
