// kernels_jpegdec.hpp -- baseline JPEG streams in device memory -> RGB24 frames in the chunk staging layout the images entries read.
// Included by yolo2_jpegdec.hip only.  The arithmetic is jpeg_scan.hpp's (shared with the host doorway); this file is the mapping of
// that work onto the machine:
//   k_jpegdec_entropy   one lane per restart interval: Huffman decode + dequantisation into the frame's coefficient blocks.  Scalar-like
//                       work on a vector machine: the lanes of a wavefront walk different streams, so every memory access is a gather and
//                       the loops run as long as the slowest lane.  Bounded by the geometry (MCUs x blocks x 64 turns), never the data.
//   k_jpegdec_idct      one thread per 8x8 block: 128 bytes of coefficients in, 64 samples out, the block in registers.
//   k_jpegdec_rgb       one thread per output pixel: up-sample + YCbCr -> RGB24 (or the grey sample three times).
//   k_jpegdec_zero      a frame whose status is not 0: its RGB24 slot zero-filled before anything reads it.
// The chunk's blob (one H2D) holds, at the offsets in JpegDecArgs: Frame[n_frames], Segment[n_seg], the table set of every workgroup of
// the entropy kernel (-1: its lanes name different sets), the status words (frames, then segments), Tables[], then the streams.
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_scan.hpp"

namespace y2jpg {

struct JpegDecArgs {
    const uint8_t *blob;           // 256-byte aligned; Segment::begin / end are offsets into it
    uint32_t frames_off, segs_off, wg_off, status_off, tables_off;
    int n_frames, n_seg;
    int16_t *coef;                 // zeroed in front of the entropy kernel
    uint8_t *planes;
    uint8_t *rgb;                  // the chunk's device staging buffer; Frame::rgb_off is relative to it
};

constexpr int kEntropyLanes = 64;  // one wavefront per workgroup: a table set in LDS (9.1 KB) serves 64 segments

__global__ __launch_bounds__(kEntropyLanes) void k_jpegdec_entropy(JpegDecArgs a)
{
    __shared__ uint4 lds_tables[sizeof(Tables) / 16];
    const Frame *frames = reinterpret_cast<const Frame *>(a.blob + a.frames_off);
    const Segment *segs = reinterpret_cast<const Segment *>(a.blob + a.segs_off);
    const Tables *tables = reinterpret_cast<const Tables *>(a.blob + a.tables_off);
    const int wg_set = reinterpret_cast<const int *>(a.blob + a.wg_off)[blockIdx.x];
    if (wg_set >= 0) {             // (uniform) every lane of this workgroup reads the same set: from LDS
        const uint4 *src = reinterpret_cast<const uint4 *>(tables + wg_set);
        for (unsigned i = threadIdx.x; i < sizeof(Tables) / 16; i += kEntropyLanes) lds_tables[i] = src[i];
        __syncthreads();
    }
    const int i = (int)(blockIdx.x * kEntropyLanes + threadIdx.x);
    if (i >= a.n_seg) return;
    const Segment s = segs[i];
    const Frame &f = frames[s.frame];
    const Tables *t = wg_set >= 0 ? reinterpret_cast<const Tables *>(lds_tables) : tables + f.tables;
    const int st = decode_segment(f, *t, a.blob, s, a.coef + f.coef_off);
    if (st) reinterpret_cast<int *>(const_cast<uint8_t *>(a.blob) + a.status_off)[a.n_frames + i] = st;   // the lane's own word
}

constexpr int kIdctThreads = 64;

// grid (ceil(most blocks of a frame / 64), n_frames)
__global__ __launch_bounds__(kIdctThreads) void k_jpegdec_idct(JpegDecArgs a)
{
    const Frame &f = reinterpret_cast<const Frame *>(a.blob + a.frames_off)[blockIdx.y];
    const int j = (int)(blockIdx.x * kIdctThreads + threadIdx.x);
    if (j >= f.blocks) return;
    int k = 0;
    if (f.ncomp == 3) k = (uint32_t)j * 64u >= f.comp[2].off ? 2 : ((uint32_t)j * 64u >= f.comp[1].off ? 1 : 0);
    const Comp &c = f.comp[k];
    const int local = j - (int)(c.off / 64u), bw = c.w2 >> 3, bx = local % bw, by = local / bw;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.coef + f.coef_off + (size_t)j * 64);   // (coef_off is a multiple of 64)
    int16_t d[64];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 w = src[q];
        d[q * 8 + 0] = (int16_t)(w.x & 0xffffu); d[q * 8 + 1] = (int16_t)(w.x >> 16);
        d[q * 8 + 2] = (int16_t)(w.y & 0xffffu); d[q * 8 + 3] = (int16_t)(w.y >> 16);
        d[q * 8 + 4] = (int16_t)(w.z & 0xffffu); d[q * 8 + 5] = (int16_t)(w.z >> 16);
        d[q * 8 + 6] = (int16_t)(w.w & 0xffffu); d[q * 8 + 7] = (int16_t)(w.w >> 16);
    }
    idct_block(a.planes + f.plane_off + c.off + (size_t)by * 8 * c.w2 + (size_t)bx * 8, c.w2, d);
}

constexpr int kRgbThreads = 256;

// grid (ceil(most pixels of a frame / 256), n_frames)
__global__ __launch_bounds__(kRgbThreads) void k_jpegdec_rgb(JpegDecArgs a)
{
    const Frame &f = reinterpret_cast<const Frame *>(a.blob + a.frames_off)[blockIdx.y];
    if (f.raw) return;
    const unsigned p = blockIdx.x * kRgbThreads + threadIdx.x;
    if (p >= (unsigned)f.width * (unsigned)f.height) return;
    const int y = (int)(p / (unsigned)f.width), x = (int)(p - (unsigned)y * (unsigned)f.width);
    uint8_t px[3];
    rgb_pixel(f, a.planes + f.plane_off, x, y, px);
    uint8_t *out = a.rgb + f.rgb_off + (size_t)p * 3;
    out[0] = px[0]; out[1] = px[1]; out[2] = px[2];
}

// grid (blocks, n_frames): the frame's status words (its own, then its segments') reduced by every workgroup; a flagged frame's slot
// is written with zeros (grid-stride).  Plain vector stores.
__global__ __launch_bounds__(256) void k_jpegdec_zero(JpegDecArgs a)
{
    const Frame &f = reinterpret_cast<const Frame *>(a.blob + a.frames_off)[blockIdx.y];
    if (f.raw) return;
    const int *status = reinterpret_cast<const int *>(a.blob + a.status_off);
    int bad = status[blockIdx.y];
    for (int s = (int)threadIdx.x; s < f.n_seg; s += 256) bad |= status[a.n_frames + f.first_seg + s];
    if (!__syncthreads_or(bad)) return;
    const size_t bytes = (size_t)f.width * f.height * 3;
    uint8_t *out = a.rgb + f.rgb_off;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < bytes; i += (size_t)gridDim.x * 256) out[i] = 0;
}

}  // namespace y2jpg
