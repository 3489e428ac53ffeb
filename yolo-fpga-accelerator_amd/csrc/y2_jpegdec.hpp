// y2_jpegdec.hpp -- the GPU JPEG decoder as one stage of a chunk loop (yolo2_jpegdec.hip): what the chunk loop of the decode / records
// entries (run_jpeg) and the loop entry from streams (yolo2_loop.hip) both call.  The caller owns the chunk loop, the staging layout
// and every other stream operation; this stage owns the headers, the chunk's blob (PipeBufs::hjpg / djpg), the decoder launches and
// the status words.  Per chunk k, buffer set b = k & 1, in this order:
//   _stage      host: the blob of chunk k with every frame's RGB24 slot at slot[f] of dbytes[b]; the caller's raw frames copied to
//               hin + slot[f]; then the blob's H2D on s_in
//   _upload_raw the raw frames' H2Ds on s_in (each into its slot of dbytes[b])
//   _launch     on s_run, which the caller has made wait for the uploads: coefficient memset, entropy stage (option jpegdec_split:
//               k_jpegdec_split + k_jpegdec_rest), k_jpegdec_idct, _rgb, _zero
//   _status_d2h the status words' D2H on the stream given (behind everything that waits for the decoder)
//   _collect    host, once that copy has been waited for: per-frame status
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>

#include <hip/hip_runtime.h>

struct yolo2_hip_ctx;
struct Y2JpegDec;
struct Y2JpegDecDelete { void operator()(Y2JpegDec *d) const; };
typedef std::unique_ptr<Y2JpegDec, Y2JpegDecDelete> Y2JpegDecPtr;

// The headers of n streams (sizes[i] == 0 with raw_ok: frame i is raw RGB24 of widths[i] x heights[i]); widths / heights are filled
// for the others.  check(i) runs behind frame i's header and may refuse it.  Reads option jpegdec_split.  No GPU call; c may be
// nullptr where only the refusals are wanted.
int y2_jpegdec_open(yolo2_hip_ctx *c, const uint8_t *const *streams, const size_t *sizes, int *widths, int *heights, int n, bool raw_ok,
                    const std::function<int(int)> &check, Y2JpegDecPtr *out);
// the chunks of `batch` frames: the largest blob, coefficient count and status words (refuses a chunk past 2 GiB); no GPU call
int y2_jpegdec_plan(Y2JpegDec *d, int batch);
// grows PipeBufs' JPEG buffers to the plan and makes the timing events (after y2_pipe_ensure: growing that drops these)
int y2_jpegdec_ensure(Y2JpegDec *d);
bool y2_jpegdec_raw(const Y2JpegDec *d, int frame);
int y2_jpegdec_stage(Y2JpegDec *d, int k, const size_t *slot, uint8_t *hin);
int y2_jpegdec_upload_raw(Y2JpegDec *d, int k, const size_t *slot, const uint8_t *hin);
int y2_jpegdec_launch(Y2JpegDec *d, int k);
int y2_jpegdec_status_d2h(Y2JpegDec *d, int k, hipStream_t st);
void y2_jpegdec_collect(Y2JpegDec *d, int k, int *status, int *first_bad);
// what yolo2_hip_jpeg_last_info / _split_info report: the event times, the blob and raw-frame bytes uploaded plus `other_bytes`
void y2_jpegdec_close(Y2JpegDec *d, double other_bytes);
double y2_jpegdec_uploaded(const Y2JpegDec *d);   // blob and raw-frame bytes so far
