// kernels_i8_front_pix.hpp -- the front of the int8 pass (kernels_i8_front.hpp) from a chunk of planar YUV 4:2:0 frames: i8_front_tiles
// with the LbYuv420 fetch (letterbox.hpp), one kernel per format under its own name.  Everything after the fetch is the template's:
// the tensor is bit-identical to k_i8_front_u8's on the converted RGB24 frames (tests/test_gpu_yuv420.py).
#pragma once
#include "kernels_i8_front.hpp"

namespace y2 {

// k_i8_front_<short> of every kind whose I8 column says GEN (pix_formats.hpp; the TPL kinds are k_i8_front_pix<fetch> itself).
// Bit-identical to k_i8_front_u8's on the reordered bytes (packed: tests/test_gpu_packed.py) or on the demosaiced frame (raw Bayer:
// tests/test_gpu_bayer.py).
#define Y2_I8F_TPL(SHORT, ...)
#define Y2_I8F_GEN(SHORT, ...) \
    __global__ __launch_bounds__(256) void k_i8_front_##SHORT(const FrontI8Args a) { i8_front_tiles<__VA_ARGS__>(a); }
#define Y2_I8F_ROW(KIND, SHORT, LB, I8, F16, ...) Y2_I8F_##I8(SHORT, __VA_ARGS__)
Y2_PIX_KINDS(Y2_I8F_ROW)
#undef Y2_I8F_ROW
#undef Y2_I8F_GEN
#undef Y2_I8F_TPL

}  // namespace y2
