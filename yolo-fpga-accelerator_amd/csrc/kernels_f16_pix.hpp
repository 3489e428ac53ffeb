// kernels_f16_pix.hpp -- layers 0+1 of the fp16 / split-fp16 pass straight from a chunk of planar YUV 4:2:0 frames: kernels_f16.hpp's
// conv0_pool_mfma_tiles<SPLIT, U8, PIX> with the LbYuv420 fetch (letterbox.hpp).  Two more instantiations beside k_conv0_pool_mfma_u8
// and k_conv0_pool_mfma_yuyv, so that no kernel pays for a format it is not reading; everything after the fetch is the template's, so
// the output is bit-identical to k_letterbox_nv12_batch / k_letterbox_i420_batch followed by k_conv0_pool_mfma (tests/test_gpu_yuv420.py).
// Include AFTER kernels_f16.hpp.
#pragma once
#include "kernels_f16.hpp"

namespace y2 {

// NV12: Y plane, then interleaved U V pairs of every 2 x 2 block
template <bool SPLIT = false>
__global__ __launch_bounds__(256) void k_conv0_pool_mfma_nv12(const uint8_t *__restrict__ lb, int lb_first, const float *__restrict__ w0,
                                                               const float *__restrict__ bias0, _Float16 *__restrict__ out, int oWp, int oPL,
                                                               int n_tile_total)
{
    conv0_pool_mfma_tiles<SPLIT, true, LbYuv420<true>>(nullptr, lb, lb_first, w0, bias0, out, 416, 416, oWp, oPL, n_tile_total);
}

// I420 (yuv420p): Y plane, U plane, V plane
template <bool SPLIT = false>
__global__ __launch_bounds__(256) void k_conv0_pool_mfma_i420(const uint8_t *__restrict__ lb, int lb_first, const float *__restrict__ w0,
                                                               const float *__restrict__ bias0, _Float16 *__restrict__ out, int oWp, int oPL,
                                                               int n_tile_total)
{
    conv0_pool_mfma_tiles<SPLIT, true, LbYuv420<false>>(nullptr, lb, lb_first, w0, bias0, out, 416, 416, oWp, oPL, n_tile_total);
}

// Packed RGB in another byte order or with a fourth byte (LbPacked): BGR24, RGBA32, BGRA32.  The permutation is at the fetch, not in
// layer 0's weights: the k order inside the MFMA, and with it every fp16 bit, is k_conv0_pool_mfma_u8's (tests/test_gpu_packed.py).
#define Y2_CONV0_PACKED(NAME, BPP, SWAP)                                                                                                   \
    template <bool SPLIT = false>                                                                                                          \
    __global__ __launch_bounds__(256) void NAME(const uint8_t *__restrict__ lb, int lb_first, const float *__restrict__ w0,               \
                                                const float *__restrict__ bias0, _Float16 *__restrict__ out, int oWp, int oPL,            \
                                                int n_tile_total)                                                                          \
    {                                                                                                                                      \
        conv0_pool_mfma_tiles<SPLIT, true, LbPacked<BPP, SWAP>>(nullptr, lb, lb_first, w0, bias0, out, 416, 416, oWp, oPL, n_tile_total); \
    }
Y2_CONV0_PACKED(k_conv0_pool_mfma_bgr24, 3, true)
Y2_CONV0_PACKED(k_conv0_pool_mfma_rgba32, 4, false)
Y2_CONV0_PACKED(k_conv0_pool_mfma_bgra32, 4, true)
#undef Y2_CONV0_PACKED

}  // namespace y2
