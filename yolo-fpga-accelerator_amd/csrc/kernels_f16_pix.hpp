// kernels_f16_pix.hpp -- layers 0+1 of the fp16 / split-fp16 pass straight from a chunk of planar YUV 4:2:0 frames: kernels_f16.hpp's
// conv0_pool_mfma_tiles<SPLIT, U8, PIX> with the LbYuv420 fetch (letterbox.hpp).  Two more instantiations beside k_conv0_pool_mfma_u8
// and k_conv0_pool_mfma_yuyv, so that no kernel pays for a format it is not reading; everything after the fetch is the template's, so
// the output is bit-identical to k_letterbox_nv12_batch / k_letterbox_i420_batch followed by k_conv0_pool_mfma (tests/test_gpu_yuv420.py).
// Include AFTER kernels_f16.hpp.
#pragma once
#include "kernels_f16.hpp"

namespace y2 {

// k_conv0_pool_mfma_<short> of every kind whose F16 column says GEN (pix_formats.hpp).  For the packed formats the permutation is at
// the fetch, not in layer 0's weights: the k order inside the MFMA, and with it every fp16 bit, is k_conv0_pool_mfma_u8's
// (tests/test_gpu_packed.py).
#define Y2_CONV0_HAS(SHORT, ...)
#define Y2_CONV0_NONE(SHORT, ...)
#define Y2_CONV0_GEN(SHORT, ...)                                                                                                               \
    template <bool SPLIT = false>                                                                                                          \
    __global__ __launch_bounds__(256) void k_conv0_pool_mfma_##SHORT(const uint8_t *__restrict__ lb, int lb_first, const float *__restrict__ w0, \
                                                const float *__restrict__ bias0, _Float16 *__restrict__ out, int oWp, int oPL,            \
                                                int n_tile_total)                                                                          \
    {                                                                                                                                      \
        conv0_pool_mfma_tiles<SPLIT, true, __VA_ARGS__>(nullptr, lb, lb_first, w0, bias0, out, 416, 416, oWp, oPL, n_tile_total);         \
    }
#define Y2_CONV0_ROW(KIND, SHORT, LB, I8, F16, ...) Y2_CONV0_##F16(SHORT, __VA_ARGS__)
Y2_PIX_KINDS(Y2_CONV0_ROW)
#undef Y2_CONV0_ROW
#undef Y2_CONV0_GEN
#undef Y2_CONV0_NONE
#undef Y2_CONV0_HAS

}  // namespace y2
