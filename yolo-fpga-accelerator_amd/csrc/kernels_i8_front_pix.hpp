// kernels_i8_front_pix.hpp -- the front of the int8 pass (kernels_i8_front.hpp) from a chunk of planar YUV 4:2:0 frames: i8_front_tiles
// with the LbYuv420 fetch (letterbox.hpp), one kernel per format under its own name.  Everything after the fetch is the template's:
// the tensor is bit-identical to k_i8_front_u8's on the converted RGB24 frames (tests/test_gpu_yuv420.py).
#pragma once
#include "kernels_i8_front.hpp"

namespace y2 {

__global__ __launch_bounds__(256) void k_i8_front_nv12(const FrontI8Args a) { i8_front_tiles<LbYuv420<true>>(a); }
__global__ __launch_bounds__(256) void k_i8_front_i420(const FrontI8Args a) { i8_front_tiles<LbYuv420<false>>(a); }
// packed BGR24 / RGBA32 / BGRA32 frames (LbPacked): bit-identical to k_i8_front_u8's on the reordered bytes (tests/test_gpu_packed.py)
__global__ __launch_bounds__(256) void k_i8_front_bgr24(const FrontI8Args a) { i8_front_tiles<LbPacked<3, true>>(a); }
__global__ __launch_bounds__(256) void k_i8_front_rgba32(const FrontI8Args a) { i8_front_tiles<LbPacked<4, false>>(a); }
__global__ __launch_bounds__(256) void k_i8_front_bgra32(const FrontI8Args a) { i8_front_tiles<LbPacked<4, true>>(a); }

}  // namespace y2
