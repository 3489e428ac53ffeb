// kernels_pix.hpp -- kernels_pre.hpp's letterbox kernels for camera pixel formats other than interleaved bytes: packed YUYV 4:2:2
// frames (V4L2 'YUYV', 2 bytes per pixel) -> letterboxed float frame, for the int16 images entries, the f16_no_mfma0 route of the
// fp16 ones and yolo2_hip_letterbox_pix.
//
// The reference's camera loop turns a YUYV frame into RGB24 on the host (yolo2_yuyv_to_rgb24, linux_app/src/yolo2_v4l2.c:328-374)
// before rgb24_to_chw_float and letterbox_image; here every fetched pixel is converted where it is read (LbYuyv, letterbox.hpp),
// so two bytes per pixel cross PCIe instead of three and no host thread touches them.  The float operations after the fetch are
// lb_part's / lb_value's (letterbox.hpp restates them with the fetch as a parameter): the frame is bit-identical to
// k_letterbox_u8's on the converted RGB24 image (tests/test_gpu_yuyv.py).
//
// NV12 and I420 frames (planar YUV 4:2:0, what video decoders emit) go the same way through LbYuv420: k_letterbox_nv12[_batch] and
// k_letterbox_i420[_batch], 1.5 bytes per pixel (tests/test_gpu_yuv420.py).
//
// Packed BGR24, RGBA32 and BGRA32 frames (what OpenCV, GUI toolkits and screen capture hold) go through LbPacked, which only picks
// another byte: k_letterbox_bgr24[_batch], k_letterbox_rgba32[_batch], k_letterbox_bgra32[_batch] (tests/test_gpu_packed.py).
//
// Include AFTER kernels_pre.hpp, in the one translation unit that includes it (yolo2_hip.hip): LetterboxArgs / LetterboxItem are
// kernels_pre.hpp's definitions there, and letterbox.hpp's restatement of them is switched off.
#pragma once
#define Y2_LETTERBOX_STRUCTS_FROM_PRE
#include "letterbox.hpp"

namespace y2 {

template <class PIX>
__device__ inline float lb_value_pix(const uint8_t *__restrict__ img, const LetterboxArgs &a, int t)
{
    const int plane = a.net_w * a.net_h;
    const int k = t / plane, rem = t - k * plane;
    const int y = rem / a.net_w;
    return lb_value_at<LbDiv255, PIX>(img, a, k, y, rem - y * a.net_w);
}
__device__ inline float lb_value_yuyv(const uint8_t *__restrict__ img, const LetterboxArgs &a, int t) { return lb_value_pix<LbYuyv>(img, a, t); }

// one image (a.ch == 2, a.w even, img on a 4-byte boundary)
__global__ void k_letterbox_yuyv(const uint8_t *__restrict__ img, float *__restrict__ out, const LetterboxArgs a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * a.net_w * a.net_h) return;
    out[t] = lb_value_yuyv(img, a, t);
}

// a whole chunk (k_letterbox_u8_batch's staging buffer: the LetterboxItem table, then the frames; blockIdx.y = frame)
__global__ void k_letterbox_yuyv_batch(const uint8_t *__restrict__ base, float *__restrict__ out, int frame_elems)
{
    const LetterboxItem *it = reinterpret_cast<const LetterboxItem *>(base) + blockIdx.y;
    const LetterboxArgs a = it->a;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * a.net_w * a.net_h) return;
    out[(size_t)blockIdx.y * frame_elems + t] = lb_value_yuyv(base + it->off, a, t);
}

// the two kernels above for a planar 4:2:0 fetch (a.w and a.h even, img at any address)
template <class PIX>
__device__ inline void letterbox_pix_one(const uint8_t *__restrict__ img, float *__restrict__ out, const LetterboxArgs &a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * a.net_w * a.net_h) return;
    out[t] = lb_value_pix<PIX>(img, a, t);
}
template <class PIX>
__device__ inline void letterbox_pix_batch(const uint8_t *__restrict__ base, float *__restrict__ out, int frame_elems)
{
    const LetterboxItem *it = reinterpret_cast<const LetterboxItem *>(base) + blockIdx.y;
    const LetterboxArgs a = it->a;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * a.net_w * a.net_h) return;
    out[(size_t)blockIdx.y * frame_elems + t] = lb_value_pix<PIX>(base + it->off, a, t);
}
__global__ void k_letterbox_nv12(const uint8_t *__restrict__ img, float *__restrict__ out, const LetterboxArgs a) { letterbox_pix_one<LbYuv420<true>>(img, out, a); }
__global__ void k_letterbox_i420(const uint8_t *__restrict__ img, float *__restrict__ out, const LetterboxArgs a) { letterbox_pix_one<LbYuv420<false>>(img, out, a); }
__global__ void k_letterbox_nv12_batch(const uint8_t *__restrict__ base, float *__restrict__ out, int frame_elems)
{
    letterbox_pix_batch<LbYuv420<true>>(base, out, frame_elems);
}
__global__ void k_letterbox_i420_batch(const uint8_t *__restrict__ base, float *__restrict__ out, int frame_elems)
{
    letterbox_pix_batch<LbYuv420<false>>(base, out, frame_elems);
}

// ... and for packed BGR24 / RGBA32 / BGRA32 frames (LbPacked: BGR24 at any address, the 32-bit formats on a 4-byte boundary)
#define Y2_LETTERBOX_PACKED(NAME, BPP, SWAP)                                                                                                  \
    __global__ void NAME(const uint8_t *__restrict__ img, float *__restrict__ out, const LetterboxArgs a)                                    \
    {                                                                                                                                         \
        letterbox_pix_one<LbPacked<BPP, SWAP>>(img, out, a);                                                                                  \
    }                                                                                                                                         \
    __global__ void NAME##_batch(const uint8_t *__restrict__ base, float *__restrict__ out, int frame_elems)                                 \
    {                                                                                                                                         \
        letterbox_pix_batch<LbPacked<BPP, SWAP>>(base, out, frame_elems);                                                                     \
    }
Y2_LETTERBOX_PACKED(k_letterbox_bgr24, 3, true)
Y2_LETTERBOX_PACKED(k_letterbox_rgba32, 4, false)
Y2_LETTERBOX_PACKED(k_letterbox_bgra32, 4, true)
#undef Y2_LETTERBOX_PACKED

}  // namespace y2
