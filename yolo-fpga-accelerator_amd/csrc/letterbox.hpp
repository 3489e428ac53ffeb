// letterbox.hpp -- kernels_pre.hpp's letterbox arithmetic for k_conv0_pool_mfma_u8 (kernels_f16.hpp), which builds layer 0's input
// patches from image bytes.  kernels_pre.hpp defines its kernels in the header, so only one translation unit (yolo2_hip.hip) may
// include it, and it is one of the int16 device sources bench.py hashes against the committed traffic measurement: it stays as it
// is.  This header restates its two structs token for token (tests/test_images_f16_abi.py compares them) and its lb_part / lb_value
// with the byte -> v / 255 step as a parameter, so that the fused kernel can take it from a table in LDS.  Every float operation
// is lb_part / lb_value's, in their order: the values are bit-identical (tests/test_gpu_images_f16.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace y2 {

struct LetterboxArgs {
    int w, h, ch;          // source image: w x h, ch interleaved byte channels (1 or 3)
    int net_w, net_h;      // canvas (416 x 416)
    int new_w, new_h;      // fitted size
    int off_x, off_y;      // where the fitted image sits on the canvas
    float w_scale, h_scale;
};

// byte -> v / 255.f as load_image_stb computes it
struct LbDiv255 {
    __device__ float operator()(uint8_t v) const { return __fdiv_rn((float)v, 255.f); }
};
// the same values from a 256-entry table of LbDiv255's results (k_conv0_pool_mfma_u8 keeps it in LDS): same bits, no division
struct LbTable {
    const float *t;
    __device__ float operator()(uint8_t v) const { return t[v]; }
};

// kernels_pre.hpp's lb_part: the horizontally interpolated value part(c, r, k) of resize_image's first pass
template <class Q = LbDiv255>
__device__ inline float lb_part_q(const uint8_t *__restrict__ img, const LetterboxArgs &a, int c, int r, int k, Q q = Q())
{
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

// kernels_pre.hpp's lb_value for canvas element (k, y, x): 0.5 outside the fitted image, resize_image's second pass inside it
template <class Q = LbDiv255>
__device__ inline float lb_value_at(const uint8_t *__restrict__ img, const LetterboxArgs &a, int k, int y, int x, Q q = Q())
{
    const int c = x - a.off_x, r = y - a.off_y;
    float v = .5f;
    if (c >= 0 && c < a.new_w && r >= 0 && r < a.new_h) {
        const float sy = __fmul_rn((float)r, a.h_scale);
        const int iy = (int)sy;
        const float dy = __fsub_rn(sy, (float)iy);
        v = __fmul_rn(__fsub_rn(1.f, dy), lb_part_q(img, a, c, min(iy, a.h - 1), k, q));
        if (!(r == a.new_h - 1 || a.h == 1)) v = __fadd_rn(v, __fmul_rn(dy, lb_part_q(img, a, c, min(iy + 1, a.h - 1), k, q)));
    }
    return v;
}

// one frame of a chunk's staging buffer: where the image's bytes start (relative to the buffer) and its geometry
struct LetterboxItem {
    unsigned long long off;
    LetterboxArgs a;
};

}  // namespace y2
