// y2_png.hpp -- what yolo2_png.hip offers batched entries beside the C ABI: the device encoder of zlib streams (dynamic-Huffman
// deflate without LZ matches, csrc/png_huff.hpp) from bytes that already lie in device memory, as a plan and one enqueue.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

struct Y2PngIn {
    size_t n;         // bytes to deflate
    size_t src_off;   // the bytes from the source base address (any alignment)
    size_t out_off;   // the stream from the output base address (any alignment); yolo2_hip_zlib_huff_bound(n) bytes are its room
};
struct Y2PngPlan {
    int nf = 0;
    std::vector<uint8_t> table;   // PngStream[nf] (kernels_png.hpp): what goes up before the launches
    size_t work_bytes = 0;        // the work area: everything below, at these offsets
    size_t hist = 0, codes = 0, hdr = 0, blocks = 0, state = 0, sizes = 0;
    unsigned grid_blk = 0, grid_tile = 0, total_blocks = 0;
};
// Lays the work area out and makes the table.
int y2_png_plan(const Y2PngIn *in, int nf, Y2PngPlan *plan);
// Enqueues the six launches on `st`: bytes at src_base + src_off -> streams at out_base + out_off, sizes as unsigned long long [nf]
// at work + plan.sizes.  table_dev: plan.table, uploaded.
int y2_png_enqueue(const Y2PngPlan &plan, const uint8_t *table_dev, const uint8_t *src_base, uint8_t *work, uint8_t *out_base, hipStream_t st);
