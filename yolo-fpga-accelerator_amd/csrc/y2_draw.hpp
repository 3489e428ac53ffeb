// y2_draw.hpp -- what yolo2_draw.hip offers the other translation units beside the C ABI (yolo2_multi.hip uses the C ABI only and
// does not include y2_internal.hpp).
#pragma once
#include <cstdint>

#include "../../include/yolo2_hip.h"

// Everything the batched annotate entries refuse, looked at before anything is allocated or launched (the multi entry asks for the
// whole call before it starts a shard).  YOLO2_SUCCESS, or YOLO2_ERROR with the cause in yolo2_hip_last_error.
int y2_annotate_check(const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch, const yolo2_hip_det *dets,
                      int cap_per_frame, const int *counts, float thresh, int n_labels, uint8_t *const *annotated);
// Everything the loop entries (yolo2_loop.hip) refuse that can be seen without a context.
int y2_loop_check(int precision, const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch, float thresh,
                  int flags, const yolo2_hip_det *dets, int cap_per_frame, const int *counts, int n_labels, int out_format, int quality,
                  uint8_t *const *out, const size_t *caps, const size_t *sizes);
// ... and the loop entry from JPEG streams: the probe's refusals (headers only), then y2_loop_check on the sizes the headers give.
int y2_loop_jpeg_check(int precision, const uint8_t *const *streams, const size_t *stream_sizes, const int *widths, const int *heights, int n, int batch,
                       float thresh, int flags, const yolo2_hip_det *dets, int cap_per_frame, const int *counts, int n_labels, int out_format,
                       int quality, uint8_t *const *out, const size_t *caps, const size_t *sizes, const int *status);
// The same for the JPEG entries: the checks above (the streams' pointers in place of the frames') and what the encoder refuses.
int y2_annotate_jpeg_check(const uint8_t *const *images, const int *widths, const int *heights, int pixfmt, int n, int batch,
                           const yolo2_hip_det *dets, int cap_per_frame, const int *counts, float thresh, int n_labels, uint8_t *const *jpeg,
                           const size_t *caps, size_t *sizes);
