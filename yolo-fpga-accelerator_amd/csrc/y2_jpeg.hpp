// y2_jpeg.hpp -- what yolo2_jpeg.hip offers yolo2_draw.hip (the batched annotate-and-encode entry) beside the C ABI: the device
// encoder of RGB24 frames that already lie in device memory, as a plan (sizes, offsets, grids), a table and one enqueue.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct Y2JpegFrameIn {
    int w, h;
    size_t src_off;   // the frame's RGB24 bytes from the source base address (any alignment)
    size_t cap;       // the caller's room for its stream
};
struct Y2JpegPlan {
    int nf = 0;
    size_t table_bytes = 0;   // JpegHeader + JpegFrame[nf], padded
    size_t work_bytes = 0;    // the work area: everything below, at these offsets
    size_t coef = 0, blk_off = 0, wg_sum = 0, wg_base = 0, us = 0, seg_ff = 0, seg_base = 0, state = 0, sizes = 0;
    size_t out_bytes = 0;     // sum of min(cap, bound): the most the packed output can hold
    unsigned grid_blk = 0, grid_seg = 0;
};
size_t y2_jpeg_table_bytes(int nf);
// What the encoder refuses of one frame: a width or height outside 1..65535, a bound of 2^31 bytes or more.  YOLO2_SUCCESS, or
// YOLO2_ERROR with the cause (naming frame f) in yolo2_hip_last_error.
int y2_jpeg_check_frame(int w, int h, int f);
// Checks the frames and lays the work area out.
int y2_jpeg_plan(const Y2JpegFrameIn *frames, int nf, Y2JpegPlan *plan);
// Writes the chunk's table (y2_jpeg_table_bytes(nf) bytes) for frames that y2_jpeg_plan accepted, at `quality`.
void y2_jpeg_write_table(const Y2JpegFrameIn *frames, int nf, int quality, uint8_t *table);
// Enqueues stages A - D on `st`: frames at src_base + src_off -> streams packed into out_base (frame f at the sum of
// min(size, cap) of the frames before it), sizes as unsigned long long [nf] at work + plan.sizes.  table_dev: the uploaded table.
int y2_jpeg_enqueue(const Y2JpegPlan &plan, const uint8_t *table_dev, const uint8_t *src_base, uint8_t *work, uint8_t *out_base, hipStream_t st);
