/*
 * yolo2_hip.h -- C ABI of the MI355X (gfx950) YOLOv2 accelerator library, libyolo2_hip.so.
 *
 * This is the drop-in boundary: it stands where the reference's AXI-Lite/udmabuf driver
 * stands (linux_app/include/yolo2_accel_linux.h, linux_app/include/dma_buffer_manager.h)
 * and where the host simulation calls YOLO2_FPGA (hls/models/yolov2/yolo2_accel.hpp:10-17).
 * Plain C: pointers, sizes and ints only; no C++ exceptions cross it; every entry point
 * returns one of the reference's status codes (linux_app/include/yolo2_config.h:146-151).
 *
 * "Physical address" in the reference == a device-accessible address here (uint64_t):
 * either HBM from yolo2_hip_alloc(), or mapped pinned host memory from memory_allocate_*().
 *
 * Three tiers, innermost first:
 *   1. driver + per-layer calls with the reference's exact argument lists and DRAM layouts
 *      (feature maps [C][H][W8], weights in weights_reorg order) -- lets the reference's C
 *      layer loop (linux_app/src/yolo2_inference.c:763-910) drive the GPU unchanged;
 *   2. whole-network batched entry: weights resident in HBM, 28 layer kernels per batch
 *      on one stream, one host sync per batch instead of one per layer;
 *   3. helpers the callers on either side need (weight-file quirks, region gather).
 */
#ifndef YOLO2_HIP_H
#define YOLO2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* linux_app/include/yolo2_config.h:146-151 */
#define YOLO2_SUCCESS     0
#define YOLO2_ERROR      -1
#define YOLO2_TIMEOUT    -2
#define YOLO2_INIT_ERROR -3
#define YOLO2_MMAP_ERROR -4   /* here: allocation / mapping failure */
#define YOLO2_DMA_ERROR  -5   /* here: host<->device copy failure */

/* ------------------------------------------------------------------ tier 1: driver */

/* yolo2_accel_init / yolo2_accel_cleanup (yolo2_accel_linux.h:19-31).  Binds the calling
 * process to the HIP device selected by yolo2_hip_select_device() (default 0). */
int  yolo2_accel_init(void);
void yolo2_accel_cleanup(void);
int  yolo2_hip_select_device(int device);
int  yolo2_hip_device_count(void);
const char *yolo2_hip_last_error(void);

/* yolo2_set_q_values (yolo2_accel_linux.h:33-41): the reference latches Q values in AXI
 * GPIOs; the per-layer calls below also take them as arguments, which win. */
void yolo2_set_q_values(int32_t qw, int32_t qa_in, int32_t qa_out, int32_t qb);
int  yolo2_is_busy(void);                            /* yolo2_accel_linux.h:43-47 */
int  yolo2_is_done(void);                            /* :49-53 */
int  yolo2_wait_for_completion(uint32_t timeout_ms); /* :55-61 */

/* yolo2_get_status / yolo2_read_reg / yolo2_write_reg (yolo2_accel_linux.h:57-61, 123-134).  The
 * reference exposes the HLS IP's AXI-Lite register file (offsets: linux_app/include/yolo2_config.h:
 * 36-71).  Here it is a 4 KiB shadow register file with the same offsets: the per-layer calls latch
 * their addresses and scalars into it exactly like yolo2_accel_linux.c:446-505 writes them, AP_CTRL
 * (offset 0) reads ap_done|ap_idle|ap_ready (0x0e) while the device is idle and ap_start (0x01)
 * while a layer is in flight, and writing ap_start to AP_CTRL runs the layer the registers describe
 * (conv for LayerType 0, maxpool for 1) with the Q values of yolo2_set_q_values(), blocking.
 * All three return 0 / do nothing before yolo2_accel_init(), like the reference. */
uint32_t yolo2_get_status(void);
uint32_t yolo2_read_reg(uint32_t offset);
void     yolo2_write_reg(uint32_t offset, uint32_t value);
/* Per-layer calls (conv + maxpool) served since yolo2_accel_init(): the reference's layer loop
 * (linux_app/src/yolo2_inference.c:763-910) makes 28 per frame. */
long yolo2_hip_driver_calls(void);

/* yolo2_execute_conv_layer (yolo2_accel_linux.h:70-99).  Same 27 arguments and meaning as
 * YOLO2_FPGA with LayerType 0.  input/output are [C][H][W8] int16, weight is the layer's
 * slice of weights_reorg_int16 (blocks of TM x TN x K*K), beta the layer's int16 biases.
 * tm/tn/tr/tc/ofm_num_bound/mloops* are validated like yolo2_accel_linux.c:383-414 and
 * otherwise unused (GPU tiling is internal and does not change results).  Blocking. */
int yolo2_execute_conv_layer(uint64_t input_addr, uint64_t output_addr, uint64_t weight_addr,
                             uint64_t beta_addr, int ifm_num, int ofm_num, int ksize, int kstride,
                             int input_w, int input_h, int output_w, int output_h, int padding,
                             int is_nl, int is_bn, int tm, int tn, int tr, int tc, int ofm_num_bound,
                             int mloopsxTM, int mloops_a1xTM, int layer_type, int qw, int qa_in,
                             int qa_out, int qb, uint32_t timeout_ms);

/* yolo2_execute_maxpool_layer (yolo2_accel_linux.h:104-121). */
int yolo2_execute_maxpool_layer(uint64_t input_addr, uint64_t output_addr, int channels, int ksize,
                                int kstride, int input_w, int input_h, int output_w, int output_h,
                                int padding, int tm, int tr, int tc, int ofm_num_bound, int mloopsxTM,
                                int mloops_a1xTM, uint32_t timeout_ms);

/* Arithmetic form the most recent yolo2_execute_conv_layer ran (codes of yolo2_hip_layer_path below;
 * -1 = the generic one-thread-per-output kernel for shapes the tiled kernel does not cover).  The
 * per-layer calls prove the form for the whole layer from the weights and Q values of that call. */
int yolo2_hip_last_layer_path(void);
/* 1 if the last int16 conv of the driver tier ran edge-class pixel tiles (yolo2_hip_i16_edge_map), else 0. */
int yolo2_hip_last_layer_edge(void);

/* fp32 twin of the conv call (host-sim form YOLO2_FPGA without INT16_MODE,
 * hls/models/yolov2/yolo2_accel.hpp:10-17): float tensors, Q arguments absent. */
int yolo2_execute_conv_layer_f32(uint64_t input_addr, uint64_t output_addr, uint64_t weight_addr,
                                 uint64_t beta_addr, int ifm_num, int ofm_num, int ksize, int kstride,
                                 int input_w, int input_h, int output_w, int output_h, int padding,
                                 int is_nl, uint32_t timeout_ms);

/* Buffers: dma_buffer_manager.h:94-139.  ptr is CPU-visible, phys_addr GPU-visible; both
 * name the same mapped pinned pages, so flush/invalidate only have to order, not copy. */
#ifndef DMA_BUFFER_MANAGER_H   /* the reference's own header may be included first: same types */
typedef struct {
    void *ptr;
    size_t size;
    uint64_t phys_addr;
} memory_buffer_t;
/* dma_buffer_t (dma_buffer_manager.h:24-30): fd is -1 and device_name "hip-pinned" here */
typedef struct {
    void *virt_addr;
    uint64_t phys_addr;
    size_t size;
    int fd;
    char device_name[64];
} dma_buffer_t;
#endif
/* dma_buffer_init / dma_buffer_cleanup (dma_buffer_manager.h:32-42; called by the reference's main,
 * linux_app/src/main.c:572,1301): init checks that a HIP device is present (the udmabuf check of
 * dma_buffer_manager.c:137-182), cleanup frees every buffer still allocated (:184-192).
 * dma_buffer_alloc .. dma_buffer_get_phys (:44-92): the udmabuf-level interface under memory_allocate_*. */
int      dma_buffer_init(void);
void     dma_buffer_cleanup(void);
int      dma_buffer_alloc(size_t size, dma_buffer_t *buffer);
void     dma_buffer_free(dma_buffer_t *buffer);
void     dma_buffer_sync_for_device(dma_buffer_t *buffer, size_t offset, size_t size);
void     dma_buffer_sync_for_cpu(dma_buffer_t *buffer, size_t offset, size_t size);
uint64_t dma_buffer_get_phys(dma_buffer_t *buffer, size_t offset);
int      memory_allocate_ddr(size_t size, size_t alignment, memory_buffer_t *buffer);
void     memory_free_ddr(memory_buffer_t *buffer);
int      memory_allocate_weights(size_t size, memory_buffer_t *buffer);
int      memory_allocate_bias(size_t size, memory_buffer_t *buffer);
int      memory_allocate_inference_buffer(memory_buffer_t *buffer);
uint64_t memory_get_phys_addr(void *virt_addr);
void     memory_flush_cache(void *addr, size_t size);
void     memory_invalidate_cache(void *addr, size_t size);

/* HBM buffers for callers that manage residency themselves.  yolo2_hip_alloc allocates on the calling thread's CURRENT
 * device (the driver tier is a one-device interface); a caller that holds contexts on several devices uses _alloc_on. */
int  yolo2_hip_alloc(size_t bytes, uint64_t *dev_addr);
void yolo2_hip_free(uint64_t dev_addr);
int  yolo2_hip_memcpy_h2d(uint64_t dst, const void *src, size_t bytes);
int  yolo2_hip_memcpy_d2h(void *dst, uint64_t src, size_t bytes);
int  yolo2_hip_memset(uint64_t dst, int value, size_t bytes);

/* ------------------------------------------------------- tier 2: whole network, batched */

typedef struct yolo2_hip_ctx yolo2_hip_ctx; /* one per device; thread-compatible */

#define YOLO2_N_CONV       23
#define YOLO2_N_WEIGHTS    50941792   /* hls/models/yolov2/yolo2_accel.cpp:41 */
#define YOLO2_N_BIAS       10761      /* :42 */
#define YOLO2_REGION_ELEMS (425 * 13 * 13)
#define YOLO2_FRAME_ELEMS  (3 * 416 * 416)

int  yolo2_hip_create(int device, yolo2_hip_ctx **ctx);
void yolo2_hip_destroy(yolo2_hip_ctx *ctx);   /* also leaves the context's RCCL communicator, if it joined one */
int  yolo2_hip_ctx_device(yolo2_hip_ctx *ctx);
/* HBM on the context's device, whatever device the calling thread has current (and leaves that binding in force) */
int  yolo2_hip_alloc_on(yolo2_hip_ctx *ctx, size_t bytes, uint64_t *dev_addr);

/* Weights as yolov2_hls_ps holds them after load_weights (yolo2_model.cpp:158-227): the
 * weights_reorg_int16 stream with the per-layer file pad already stripped
 * (yolo2_strip_int16_layer_pad below), dense int16 biases, three int32 Q tables.
 * Uploads once, re-packs partial tiles on the device, and proves per layer which arithmetic
 * width is exact for these weights and Q values (yolo2_hip_layer_path). */
int yolo2_hip_load_weights_int16(yolo2_hip_ctx *ctx, const int16_t *weights_reorg, size_t n_weights,
                                 const int16_t *bias, size_t n_bias, const int32_t *weight_q,
                                 int n_weight_q, const int32_t *bias_q, int n_bias_q,
                                 const int32_t *act_q, int n_act_q);
/* Same, the two blobs already in HBM (e.g. received by an RCCL broadcast). */
int yolo2_hip_load_weights_int16_dev(yolo2_hip_ctx *ctx, uint64_t weights_reorg_dev, size_t n_weights,
                                     uint64_t bias_dev, size_t n_bias, const int32_t *weight_q,
                                     int n_weight_q, const int32_t *bias_q, int n_bias_q,
                                     const int32_t *act_q, int n_act_q);

/* 0 = 32-bit form A, 1 = 32-bit form B (pre-shifted accumulator), 3 = form C (packed int16
 * accumulators), 4 = form D (form C with the requantisation shift folded into pre-scaled weights),
 * 2 = 64-bit exact path, <0 = bad ordinal / not loaded.  All are bit-exact; the
 * loader picks the narrowest one it can PROVE exact for the weights and Q values at hand
 * (csrc/kernels_int16.hpp explains the forms). */
int yolo2_hip_layer_path(yolo2_hip_ctx *ctx, int conv_ordinal);
/* The form is chosen per block of 32 output channels (a few large-weight channels must not slow
 * a whole layer down): layer_path() reports the form most blocks use, this the count per form
 * (index = the codes above). */
int yolo2_hip_layer_path_counts(yolo2_hip_ctx *ctx, int conv_ordinal, int counts[5]);

/* (Re)allocates the activation tensors for exactly `batch` frames per call. */
int yolo2_hip_set_batch(yolo2_hip_ctx *ctx, int batch);

/* One pass of the accelerator path over a batch (everything yolov2_hls_ps does between the
 * input memcpy and the region gather, yolo2_model.cpp:257-421, for `batch` frames):
 *   frames_dev  float [batch][3][416][416], letterboxed, in [0,1]  (device)
 *   region_dev  int16 [batch][425][13][13] raw region tensor       (device)
 *   *final_q    activation Q of that tensor (float = int16 * 2^-final_q)
 * Enqueues on `stream` (a hipStream_t, NULL = default stream) and returns without
 * synchronising: the caller owns the one sync per batch. */
int yolo2_hip_run_batch_int16(yolo2_hip_ctx *ctx, uint64_t frames_dev, int batch,
                              uint64_t region_dev, int *final_q, void *stream);

/* Convenience for C hosts: pageable host buffers in/out, synchronous. */
int yolo2_hip_run_batch_int16_host(yolo2_hip_ctx *ctx, const float *frames, int batch,
                                   int16_t *region, int *final_q);

/* Streaming form for hosts that hold many frames in ordinary (pageable) memory: processes
 * n_frames in chunks of `batch`, with the H2D copy of chunk k+1, the kernels of chunk k and the
 * D2H copy of chunk k-1 overlapped on three HIP streams through pinned staging buffers, so the
 * PCIe-inclusive rate approaches the device-resident rate.  Results are identical to calling
 * yolo2_hip_run_batch_int16 chunk by chunk (a trailing partial chunk is padded with the last frame). */
int yolo2_hip_run_frames_int16(yolo2_hip_ctx *ctx, const float *frames, int n_frames, int batch,
                               int16_t *region, int *final_q);

/* ---- fp16 MFMA path (floating-point form of the same network: a true dense contraction).
 * Weights as yolov2_hls_ps holds them for Precision::FP32 (weights_reorg.bin / bias.bin,
 * yolo2_model.cpp:171-181); converted once to fp16 in a K-contiguous layout on the device.
 * Activations fp16, accumulation fp32 on v_mfma_f32_32x32x16_f16, bias + leaky in fp32.
 * region_dev: float [batch][425][13][13] (what yolov2_hls_ps hands to forward_region_layer in
 * fp32 mode, yolo2_model.cpp:422-424).  Validated against the fp32 reference at box tolerance. */
int yolo2_hip_load_weights_fp32(yolo2_hip_ctx *ctx, const float *weights_reorg, size_t n_weights,
                                const float *bias, size_t n_bias);
/* Same, the two blobs already in HBM (e.g. received by the RCCL broadcast below). */
int yolo2_hip_load_weights_fp32_dev(yolo2_hip_ctx *ctx, uint64_t weights_reorg_dev, size_t n_weights,
                                    uint64_t bias_dev, size_t n_bias);
int yolo2_hip_run_batch_fp16(yolo2_hip_ctx *ctx, uint64_t frames_dev, int batch, uint64_t region_dev,
                             void *stream);
int yolo2_hip_run_batch_fp16_host(yolo2_hip_ctx *ctx, const float *frames, int batch, float *region);
/* The kernel the fp16 pass runs for layer `layer_idx` at the current batch (after the first run at that batch; "" before).
 * The selection is made ONCE per (weights, batch) into a launch table; the YOLO2_F16_* A/B switches are read when the weights
 * are loaded, never on the launch path. */
const char *yolo2_hip_fp16_layer_kernel(yolo2_hip_ctx *ctx, int layer_idx);
/* The extent check every step of that table passes before it may be launched, on explicit numbers (testable without a GPU):
 * a kernel of store kind `store` (0 = stores the full-resolution tensor only and ignores a fused pool, 1 = full-resolution or
 * pooled according to `pool`, 2 = pooled only) for a B x H x W conv writing items of Cp_out halves, channels
 * [out_ch_off, out_ch_off + n_store), into a tensor of dst_B x dst_H x dst_W pixels with dst_Cp halves per item.
 * YOLO2_SUCCESS, or YOLO2_ERROR with yolo2_hip_last_error() naming the mismatch. */
int yolo2_hip_f16_store_check(int store, int pool, int B, int H, int W, int Cp_out, int out_ch_off, int n_store, int dst_B,
                              int dst_H, int dst_W, int dst_Cp);
/* The launch table the selection makes for a plan batch, as text, without a GPU: one line per step with every field but the
 * addresses - "L<layer> <kernel> store= grid= block= lds= lt_rows= T= B= in= out= w= w2= a=<the ConvF16Args scalars> pr=<pool / reorg
 * geometry>" (tensors by the layer whose output they hold, "cat" the concat tensor; weights by conv ordinal) - then, where the images
 * entries have a layer-0 step from bytes, "u8 <kernel>" and "yuyv <kernel>".  `options` is a space-separated list of name=value
 * applied to a default option set (NULL or "": the defaults); split = 1: the fp32-tolerance pass.  Returns the length of the text
 * (buf, if not NULL, receives at most cap - 1 characters of it and a NUL), or YOLO2_ERROR for an unknown option, a value out of
 * range or a batch outside 1..4096.  A context at that batch runs this table (lanes: each at its part of the batch). */
int yolo2_hip_f16_plan_describe(const char *options, int split, int batch, char *buf, int cap);

/* Copies layer `layer_idx`'s output of frame `frame` from the last run into the reference's
 * [C][H][W8] int16 layout (pad columns zero) -- the yolov2_region_*_hw.txt style parity hook
 * (SURVEY.md section 4).  out_elems receives C*H*W8.  layer_idx -1 = the quantised network input
 * (input quantise of yolo2_model.cpp:257-273), [3][416][416]. */
int yolo2_hip_debug_layer_output(yolo2_hip_ctx *ctx, int layer_idx, int frame, int16_t *out,
                                 size_t capacity_elems, size_t *out_elems);

/* fp16 / split-fp16 parity hook: the RAW items (uint16 halves) of one frame's plane of layer `layer_idx`'s tensor from the last
 * yolo2_hip_run_batch_fp16 (split = 0) or yolo2_hip_run_batch_f32tol (split = 1), lane-aware.  which: 0 = the frame's (H+1)(W+1)
 * items, 1 = the lead items before plane 0, 2 = the tail items after the last plane (of the lane that holds the frame).
 * geom[8] = {C, Cp, H, W, Wp, items, part stride, channel offset}: items of Cp halves; split items hold [hi | lo | hi] parts of
 * `part stride` channels; layers 24 and 27 are channels 256.. / 0.. of the concat tensor.  out == NULL returns the geometry only.
 * YOLO2_ERROR for a tensor no step of the current launch table writes (fused intermediates, layer 30 = the region tensor). */
int yolo2_hip_debug_f16_tensor(yolo2_hip_ctx *ctx, int split, int layer_idx, int frame, int which, uint16_t *out,
                               size_t capacity_halves, int *geom);

/* Test hook: the bytes of device (hipMalloc) and pinned (hipHostMalloc) memory the library's contexts and calls hold right now,
 * process-wide.  Not counted: what yolo2_hip_alloc / the driver tier hand to the caller, and the process-lifetime tables and
 * scratch of the driver tier and the int16 post-processing; the per-device scratch of the synchronous yolo2_hip_postprocess_*
 * entries is counted and stays until the process ends.  (0, 0) before the first context exists. */
int yolo2_hip_debug_live_bytes(size_t *device_bytes, size_t *pinned_bytes);

/* Per-layer device time: enabling records hipEvent pairs around every layer kernel of
 * subsequent runs, on the stream they are launched on (the analogue of the per-layer latency
 * report in linux_app/src/yolo2_inference.c:75-142).  layer_times_ms returns the mean over the
 * profiled runs since the last set_profiling call (at most the latest 32). */
int yolo2_hip_set_profiling(yolo2_hip_ctx *ctx, int enable);
int yolo2_hip_layer_times_ms(yolo2_hip_ctx *ctx, float *ms32 /* [32] */);

/* A batch >= 16 runs as two, a batch of 48..127 as three part-batches ("lanes", sizes within one frame of
 * each other) on internal streams forked from and joined to the caller's stream, so that every layer is
 * several concurrent launches and one's idle tail is filled by the others (+4-6 % frames/s at batch 64).
 * Returns the lane count (1 = none).  Per-layer times and launch geometry then describe lane 0's launches. */
int yolo2_hip_num_lanes(yolo2_hip_ctx *ctx);
/* The same for the fp16 path (two half-batch lanes from batch 64; known after the first run_batch_fp16). */
int yolo2_hip_num_lanes_fp16(yolo2_hip_ctx *ctx);
/* Sets that lane count (1 = no lanes; default 2, or YOLO2_F16_LANES at weight load).  Used by bench.py to time one lane's launches
 * ALONE for the per-kernel roofline object. */
int yolo2_hip_set_fp16_lanes(yolo2_hip_ctx *ctx, int lanes);

/* ------------------------------------------------------- "fp32 fast": the matrix-core path INSIDE the fp32 tolerance
 *
 * BASELINE.json: "MFMA used only on the fp16/fp32 path where conv is a true dense contraction ... detections ... within 1e-3
 * box-coord tolerance for fp32".  The plain fp16 path is outside that tolerance (5.8e-3), the exact fp32 path is bit-identical
 * but VALU-bound.  This entry computes the reference's fp32 arithmetic (hls/core/core_compute.cpp:121-172: per output
 * bias + sum of w x, leaky x < 0 ? 0.1 x : x) on v_mfma_f32_32x32x16_f16 with every value carried as two halves
 * hi = fp16(v), lo = fp16(v - hi) and every product taken as a_hi w_hi + a_lo w_hi + a_hi w_lo (fp32 accumulate; the dropped
 * lo x lo term is 2^-22 relative): ~1e-6 relative error per layer instead of fp16's 5e-4, for 3x the MFMA work of the fp16 path.
 * Same contract as yolo2_hip_run_batch_fp16: float CHW frames in HBM -> dense fp32 [batch][425][13][13] region tensor, enqueued on
 * `stream`, needs yolo2_hip_load_weights_fp32*.  Not bit-exact with the reference (another summation order); the GPU tests hold
 * every one of the 845 boxes of the fixture frames within 1e-3 in all four coordinates (measured: ~1e-5). */
int yolo2_hip_run_batch_f32tol(yolo2_hip_ctx *ctx, uint64_t frames_dev, int batch, uint64_t region_dev, void *stream);
int yolo2_hip_run_batch_f32tol_host(yolo2_hip_ctx *ctx, const float *frames, int batch, float *region);
/* kernel the split-mode launch table runs for a layer / its lane count (after the first run at this batch) */
const char *yolo2_hip_f32tol_layer_kernel(yolo2_hip_ctx *ctx, int layer_idx);
int yolo2_hip_num_lanes_f32tol(yolo2_hip_ctx *ctx);

/* 1 when conv layer `layer_idx` (0..31) runs fused with the 2x2 max pool after it (k_conv_i16_pool: the
 * full-resolution tensor is never written, except layer 16's, which also feeds the route), 0 otherwise.
 * Chosen per batch by set_batch (timed); YOLO2_NO_POOLFUSE=1 disables, YOLO2_POOLFUSE=1 forces it wherever legal. */
int yolo2_hip_layer_pool_fused(yolo2_hip_ctx *ctx, int layer_idx);

/* Launch geometry of the conv kernel family, for the roofline report.  block = 128: k_conv_i16_w16.  pixels_per_lane = -S: the
 * layer runs k_conv_i16_ks (chain split over S workgroups).  pixels_per_lane = 0 means
 * the layer runs the split-K kernel (64/S pixels x S K-splits per wavefront, partial clamp-affine
 * maps combined with wavefront shuffles), which set_batch picks for small batches when it times
 * faster; YOLO2_SPLITK=0 / 1 in the environment disables / forces it wherever its bounds hold. */
int yolo2_hip_conv_launch_info(yolo2_hip_ctx *ctx, int conv_ordinal, int *grid_x, int *grid_y,
                               int *block, int *lds_bytes, int *pixels_per_lane);

/* The launch plan of conv layer `conv_ordinal` as text, e.g. "P=1 pad=0 w16=0 hiacc=1 ks=0 splitk=0 pp=1 grp=1 fused=0 form=4 extra=0 edge=0 xcd=4 pack=0"
 * (pixels per lane, occupancy cap, 16-channels-per-wavefront kernel, form D without v_perm, K-split over workgroups / over lanes,
 * 1x1 grouping, conv + pool fusion, arithmetic form, extra launches for blocks of another form, edge-class pixel tiles, XCD grid: 0 = none or 1 + log2 of the XCDs
 * across the channel blocks, packed triples of the lane-split kernel; new pairs are appended).  Plans come from the committed plan table (config/plan_gfx950.txt) for the batches it knows, else from timing. */
int yolo2_hip_conv_plan_string(yolo2_hip_ctx *ctx, int conv_ordinal, char *buf, int cap);
/* Where the current batch's conv plan came from: 1 = the plan table shipped next to the library (config/plan_gfx950.txt: the same
 * kernels in every process), 2 = timed in this process (a batch or a model the table does not hold, or YOLO2_AUTOTUNE=1),
 * 3 = static defaults (autotune=0), 4 = forced by a test hook (force_p), 5 = the weight-side cache bound with
 * yolo2_hip_set_plan_cache (the same kernels in every process for THIS weight set), 0 = no batch planned yet. */
int yolo2_hip_plan_source(yolo2_hip_ctx *ctx);

/* ------------------------------------------------------- options: one parsed-once set per context
 *
 * Every switch that steers kernel selection, lanes or planning is a named option of the context.  The set is filled from the
 * environment (YOLO2_<NAME>, upper case) ONCE, inside yolo2_hip_create; afterwards only this call changes it (it takes effect at the
 * next weight load / yolo2_hip_set_batch).  Nothing on a planning or launch path reads the environment.  Names (README.md has the
 * list with meanings): planning - autotune, plan_file, plan_write, lanes, no_lanes, lane_split, no_plan_cache, verbose; kernel-family
 * A/B switches - splitk, poolfuse, no_poolfuse, no_hiacc, no_ks, no_w16, no_grp, no_xcd_remap, splitk_no_pack, f16_*; test hooks
 * that force one shape everywhere - force_path, force_p, force_w16, force_hiacc, force_ks, f32_p.  value NULL or "" restores the
 * default; flags are on for any value but "0".  YOLO2_ERROR for an unknown name or a value out of range.  ctx = NULL addresses the
 * process-wide set the context-less driver tier (yolo2_execute_conv_layer ...) plans with (filled from the environment at first use).
 * (The reference's own variables - YOLO2_VERBOSE, YOLO2_NO_DUMP, YOLO2_DUMP_REGION*: linux_app/include/yolo2_log.h:27-36,
 * hls/models/yolov2/yolo2_model.cpp:427-438 - keep their names.) */
int yolo2_hip_set_option(yolo2_hip_ctx *ctx, const char *name, const char *value);
/* The options that differ from their defaults as "name=value name=value" ("" if none): what bench.py discloses with its record. */
int yolo2_hip_options_string(yolo2_hip_ctx *ctx, char *buf, int cap);

/* ------------------------------------------------------- the weight-side plan cache
 *
 * The reference prepares a weight set once, offline (src/models/yolov2/yolov2_weight_gen.cpp:34-68 writes weights_reorg*.bin;
 * the loader hls/models/yolov2/yolo2_model.cpp:158-227 only reads).  The analogue here: a small text file beside the weight set,
 * `<weights_reorg_int16.bin>.y2plan`, that this library writes the first time it has timed a batch for that weight set and reads at
 * every later load: a hash of the blobs and Q tables, the per-block bounds behind the arithmetic-form proofs (k_weight_bound* is
 * then skipped), the forms / scale shifts derived from them (re-derived and compared), and the conv plan of every timed batch as
 * plan_gfx950.txt lines (the autotune is then skipped and every process runs the same kernels).  A missing, stale (other hash),
 * damaged (checksum) or unwritable file costs time, never correctness.  weights_reorg_int16.bin stays the interchange format.
 * set_plan_cache binds the file to the context (NULL / "" unbinds) and takes effect at the next yolo2_hip_load_weights_int16*. */
int yolo2_hip_set_plan_cache(yolo2_hip_ctx *ctx, const char *path);
/* hash of the loaded weight set, whether the file's bounds were used at the last load, plan lines / batches held */
int yolo2_hip_plan_cache_info(yolo2_hip_ctx *ctx, uint64_t *weights_hash, int *bounds_from_file, int *n_lines, int *n_batches);
/* Test hook (no GPU): would the file be accepted for a weight set with this hash?  YOLO2_ERROR + the reason otherwise. */
int yolo2_hip_plan_cache_check(const char *path, uint64_t weights_hash, int *n_lines);

/* The K-split-over-workgroups kernel (k_conv_i16_ks, single frames) stores `splits` clamp-affine triples of 24 bytes per output item
 * (4 channels) and pixel into the context's scratch.  The rule every such plan passes in plan_conv and again at launch, on plain
 * numbers (no GPU): splits in {2,4,8,16} and splits x cg_out x npix x 24 <= cap_bytes; cap_bytes = 0 (a context without scratch:
 * batch > 4) refuses every split.  Round 3's GPU memory fault was this rule violated. */
int yolo2_hip_i16_plan_check(int splits, int cg_out, int npix, size_t cap_bytes);
/* Bytes of that scratch the context holds for its current batch: the largest splits x items x pixels x 24 among the plans that were
 * accepted - 0 when no layer runs the K-split kernel (round 3 held 66 MB per frame for every context of <= 4 frames). */
size_t yolo2_hip_ks_scratch_bytes(yolo2_hip_ctx *ctx);
/* Edge-class pixel tiles of the int16 3x3 conv (forms C / D, one pixel per lane): the partition of B frames of H x W pixels that the
 * kernel decodes, on plain numbers (no GPU).  Returns the number of tiles (0: the geometry keeps raster tiles); with non-null
 * arrays of room for `cap` tiles it also fills tile_cls[t] (0 top row, 1 bottom row, 2 left column, 3 right column, 4 interior,
 * 5 mixed), tile_mask[t] (the taps the tile runs, bit 3i + j for tap row i and column j) and pix[64 t + lane] (the pixel's raster
 * index (b H + y) W + x, or -1 for a padding lane), and *steps = the pixel x tap visits of the grid. */
int yolo2_hip_i16_edge_map(int B, int H, int W, int cap, int *tile_cls, int *tile_mask, int *pix, long long *steps);

/* fp32 whole network in the reference's own arithmetic (what yolov2_hls_ps does at Precision::FP32,
 * hls/models/yolov2/yolo2_model.cpp:229-449: compute() fp32 branch core_compute.cpp:121-172 in its
 * operation order without FMA contraction, pool_yolo2, the legacy reorg): one frame
 * float [3][416][416] on the host -> float [425][13][13] on the host, bit-identical to the
 * reference's region tensor, hence identical boxes (BASELINE.json asks for 1e-3).  A correctness
 * path built from the one-thread-per-output kernels; the fast floating-point path is
 * yolo2_hip_run_batch_fp16.  Needs yolo2_hip_load_weights_fp32. */
int yolo2_hip_run_frame_fp32_host(yolo2_hip_ctx *ctx, const float *frame, float *region);

/* The same exact fp32 arithmetic, batched and TILED (csrc/kernels_f32.hpp: LDS-staged input tiles, scalar weight
 * loads, P pixels x 8 channels of fp32 accumulators per lane, the reference's operation order kept product by product):
 * bit-identical to the reference's fp32 region tensor at a few hundred times the one-thread-per-output pass.
 *   frames_dev  float [batch][3][416][416]      region_dev  float [batch][425][13][13]      (device)
 * Asynchronous on `stream` like the other batched entries; the _host form is synchronous. */
int yolo2_hip_run_batch_fp32(yolo2_hip_ctx *ctx, uint64_t frames_dev, int batch, uint64_t region_dev, void *stream);
int yolo2_hip_run_batch_fp32_host(yolo2_hip_ctx *ctx, const float *frames, int batch, float *region);

/* GPU pre-processing (the step before the path): the reference host's
 * load_image_stb (bytes / 255.f, src/core/yolo_image.cpp:29-63) + letterbox_image (two-pass bilinear
 * resize_image onto a 0.5 canvas, src/core/yolo_image.cpp:84-165) as one kernel, float-for-float in
 * the reference's operation order, so the frame is bit-identical to the host code's.
 * image_dev: w x h x channels interleaved bytes (channels 1 or 3; 1 is replicated like stb's grey
 * load); frame_dev: float [3][net_h][net_w].  Asynchronous on `stream`. */
int yolo2_hip_letterbox_u8(uint64_t image_dev, int w, int h, int channels, uint64_t frame_dev,
                           int net_w, int net_h, void *stream);

/* Camera-style whole-network entry: n images of arbitrary sizes as HOST bytes -> int16 region
 * tensors [n][425][13][13] on the host, in chunks of `batch` images.  The bytes (not the 4x larger
 * float frames) cross PCIe; letterboxing runs on the GPU; upload, kernels and download of
 * consecutive chunks overlap on three HIP streams.  Synchronous. */
int yolo2_hip_run_images_u8_host(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths,
                                 const int *heights, int channels, int n, int batch,
                                 int16_t *region_host, int *final_q);

/* ------------------------------------------------------- the step after the path, on the GPU
 *
 * forward_region_layer + get_network_boxes + do_nms_sort (src/core/yolo_region.cpp:123-236, src/core/yolo_post.cpp:54-85)
 * for a whole batch, one workgroup per frame, from a region tensor that is already in HBM (the output of
 * yolo2_hip_run_batch_*).  For the int16 tensor the result is IDENTICAL to the reference host code's: every exp the
 * reference applies to one of the 65,536 possible values int16 x 2^-Q is a table the host's own libm filled, all other
 * arithmetic is IEEE +,-,*,/ in the reference's order, the per-class sort is stable like glibc's qsort.  The float entry
 * (fp16 / fp32 tensors) evaluates exp on the device: within 1 ulp of the host's.
 *   im_w / im_h [batch]   original image sizes (letterbox correction, relative = 1 like yolov2_main.cpp:310-312)
 *   dets / counts         optional: (frame, det, class, prob, box) records for every prob > 0 after NMS, in the order
 *                         the reference prints them (dets in array order, classes inner), cap_per_frame records per frame;
 *                         counts[f] = records frame f has (may exceed the cap: the surplus is dropped)
 *   rows / totals         optional: the reference's dets[] array after do_nms_sort, [batch][845][85] =
 *                         x, y, w, h, objectness, prob[80], and the number of slots in front that hold a candidate
 *   proc                  optional: l.output of forward_region_layer, [batch][425][13][13]
 * Synchronous (host buffers out): enqueues on `stream` (NULL = default) and synchronises it before returning. */
typedef struct {
    int frame, det, cls;
    float prob, x, y, w, h;
} yolo2_hip_det;
int yolo2_hip_postprocess_int16(yolo2_hip_ctx *ctx, uint64_t region_dev, int batch, int final_q, const int *im_w,
                                const int *im_h, float thresh, float nms, yolo2_hip_det *dets, int cap_per_frame,
                                int *counts, float *rows, int *totals, float *proc, void *stream);
int yolo2_hip_postprocess_f32(yolo2_hip_ctx *ctx, uint64_t region_dev, int batch, const int *im_w, const int *im_h,
                              float thresh, float nms, yolo2_hip_det *dets, int cap_per_frame, int *counts,
                              float *rows, int *totals, float *proc, void *stream);

/* The camera loop's tail.  The reference's streaming app (linux_app/src/main.c:1013-1026, :1184-1197) and its single-image mode
 * (:827-858) do not run the src/core functions above but linux_app/src/yolo2_postprocess.c, and the two do not compute the same
 * numbers.  These two entries restate that file; arguments, checks and layouts are those of the entries above, and like them each
 * enqueues on `stream` and synchronises it before returning.  What differs from the src/core tail:
 *   sigmoid      1.0f / (1.0f + expf(-x)) in float, x > 10 -> 1 and x < -10 -> 0 (:17-21), not 1. / (1. + exp(-x)) in double
 *   softmax      expf, the float sum in class order, then *= 1.0f / sum, 1 / n for a sum <= 0 (:30-57), not (float)exp(double) and / sum
 *   boxes        correct_region_boxes in float throughout, (netw - new_w) / 2.0f / netw (:77-101), not partly in double
 *   box_iou      fminf / fmaxf and * 0.5f, 0 for an overlap or a union <= 0 (:199-226)
 *   NMS          yolo2_do_nms_sort (:248-284) runs at EVERY nms, 0 (and below) included (main.c:856-858); the entries above skip
 *                the sort for nms <= 0.  The per-class sort is the same stable one; thresh < 0 stays refused.
 *   rows         the array holds only the candidates found (:153-191); the [batch][845][85] layout is kept: the first totals[f] rows
 *                are dets[] after yolo2_do_nms_sort, element for element and in its order, the rows behind them are zero
 *   proc         the `output` of yolo2_forward_region_layer
 * The int16 entry is IDENTICAL to yolo2_postprocess.c on the same tensor, by the same construction: its sigmoid and its two expf
 * are tables the host's libm filled.  The float entry evaluates expf on the device: within an ulp of the host's per value. */
int yolo2_hip_postprocess_int16_app(yolo2_hip_ctx *ctx, uint64_t region_dev, int batch, int final_q, const int *im_w,
                                    const int *im_h, float thresh, float nms, yolo2_hip_det *dets, int cap_per_frame,
                                    int *counts, float *rows, int *totals, float *proc, void *stream);
int yolo2_hip_postprocess_f32_app(yolo2_hip_ctx *ctx, uint64_t region_dev, int batch, const int *im_w, const int *im_h,
                                  float thresh, float nms, yolo2_hip_det *dets, int cap_per_frame, int *counts,
                                  float *rows, int *totals, float *proc, void *stream);

/* The whole chain for camera-style input at the path's rate: n images of arbitrary sizes as HOST bytes -> detection records, in
 * chunks of `batch` images.  Bytes cross PCIe in, letterboxing and the network run on the GPU, the region tensor STAYS in HBM and
 * the tail (region + boxes + NMS + record compaction) runs on the same device right behind the network; only the records (32 bytes
 * each) and the per-frame counts come back.  Upload, kernels and download of consecutive chunks overlap on three HIP streams.
 * What the reference's streaming loop does frame by frame on the CPU (linux_app/src/main.c:878-1288: yolo2_run_inference +
 * yolo2_forward_region_layer / get_region_detections / do_nms_sort per frame).
 *   flags   YOLO2_DETS_BEST_CLASS: one record per detection - its best class (linux_app/src/main.c:1040-1052); a frame then has at
 *           most 845 records, so cap_per_frame = 845 never truncates.  0: a record per (detection, class) with prob > 0.
 *           YOLO2_DETS_APP_TAIL: the tail is the camera loop's (yolo2_hip_postprocess_*_app above) instead of the src/core one, in
 *           every _dets entry, single- and multi-device, int16 and _f16: the records the reference's loop prints, draws and streams.
 *           Any other bit is ignored.
 *   dets    [n][cap_per_frame]; counts[f] = records frame f produced (if > cap_per_frame the surplus was dropped); dets[].frame is the
 *           image's index in `images`.  Records identical to yolo2_hip_postprocess_int16's on the same tensors.  Synchronous. */
#define YOLO2_DETS_BEST_CLASS 1
#define YOLO2_DETS_APP_TAIL 2
int yolo2_hip_run_images_u8_dets(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                 int channels, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                 int cap_per_frame, int *counts, int *final_q);

/* The same two entries on the matrix-core passes (needs yolo2_hip_load_weights_fp32): split = 0 the fp16 pass, 1 the fp32-tolerance
 * (split-fp16) pass, as in yolo2_hip_debug_f16_tensor.  Same chunks, staging, stream overlap, ragged last chunk and record layout as
 * the int16 entries; the region tensor is fp32 [n][425][13][13] and the records equal yolo2_hip_postprocess_f32's on it.  Layers 0+1
 * read the chunk's image bytes themselves (k_conv0_pool_mfma_u8): the result is bit-identical to letterboxing every image
 * (yolo2_hip_letterbox_u8) and running yolo2_hip_run_batch_fp16 / _f32tol on those frames in the same chunks. */
int yolo2_hip_run_images_u8_f16_host(yolo2_hip_ctx *ctx, int split, const uint8_t *const *images, const int *widths,
                                     const int *heights, int channels, int n, int batch, float *region_host);
int yolo2_hip_run_images_u8_dets_f16(yolo2_hip_ctx *ctx, int split, const uint8_t *const *images, const int *widths,
                                     const int *heights, int channels, int n, int batch, float thresh, float nms, int flags,
                                     yolo2_hip_det *dets, int cap_per_frame, int *counts);
/* what the last of those calls ran for layers 0+1 at that `split` ("" before the first): the fused kernel, or under the option
 * f16_no_mfma0 "k_letterbox_u8_batch + " and the frame path's layer-0 kernel */
const char *yolo2_hip_images_layer0_kernel(yolo2_hip_ctx *ctx, int split);

/* ------------------------------------------------------- camera pixel formats: the same entries with a pixel format
 *
 * The reference's camera loop (linux_app/src/main.c:942-984) takes MJPEG and YUYV from V4L2 and turns both into RGB24 on the host
 * before rgb24_to_chw_float, letterbox and inference.  These entries are the letterbox / images entries above with `int pixfmt`
 * where those have `int channels`:
 *   YOLO2_PIX_GREY8, YOLO2_PIX_RGB24   exactly the u8 entries with channels 1 / 3 (same code path, same kernels)
 *   YOLO2_PIX_YUYV                     packed YUYV 4:2:2, 2 bytes per pixel (V4L2 'YUYV' = ffmpeg yuyv422: Y0 U Y1 V per pixel
 *                                      pair), width even.  The GPU reads the YUYV bytes itself - 2 bytes per pixel cross PCIe
 *                                      and no host thread converts them - and every result is bit-identical to the RGB24
 *                                      entries on the output of the reference's yolo2_yuyv_to_rgb24
 *                                      (linux_app/src/yolo2_v4l2.c:328-374; y2h_yuyv_to_rgb24 in libyolo2_host.so restates it):
 *                                        c = Y - 16, d = U - 128, e = V - 128, arithmetic >> 8, each clamped to 0..255
 *                                        R = (298 c + 409 e + 128) >> 8
 *                                        G = (298 c - 100 d - 208 e + 128) >> 8
 *                                        B = (298 c + 516 d + 128) >> 8
 *   YOLO2_PIX_NV12, YOLO2_PIX_I420     planar YUV 4:2:0, the frames of video decoders: w * h * 3 / 2 bytes, width AND height even.
 *                                      A Y plane [h][w]; NV12 (V4L2 'NV12': hardware decoders, ISPs) follows it with one plane
 *                                      [h/2][w/2][2] of interleaved U V pairs, I420 (V4L2 'YU12' = ffmpeg yuv420p) with a U plane
 *                                      [h/2][w/2] and then a V plane [h/2][w/2].  Pixel (x, y) has Y(y, x), U(y >> 1, x >> 1) and
 *                                      V(y >> 1, x >> 1) - chroma replicated, not interpolated - and its RGB bytes are the
 *                                      formula above on those three.  Equivalently: the frame is the YUYV frame whose row y is
 *                                      Y0 U Y1 V from luma row y and chroma row y >> 1, and every result of every entry is
 *                                      bit-identical to the RGB24 entry on that frame's conversion.  This is this library's own
 *                                      extension of the reference's formula: the reference has no 4:2:0 input (its --video path
 *                                      lets ffmpeg convert), and identity with swscale's RGB is not claimed.
 *                                      y2h_yuv420_to_rgb24 in libyolo2_host.so restates it on the host.  1.5 bytes per pixel
 *                                      cross PCIe, half of RGB24's.
 *   YOLO2_PIX_BGR24                    packed B G R, 3 bytes per pixel (V4L2 'BGR3'): what OpenCV holds (cv2.VideoCapture, cv2.imread).
 *                                      Rows of w * 3 bytes, any address, no constraint on w or h.
 *   YOLO2_PIX_RGBA32, YOLO2_PIX_BGRA32 packed R G B X (V4L2 'AB24' = ffmpeg rgba / rgb0) and B G R X (V4L2 'AR24' = ffmpeg bgra / bgr0),
 *                                      4 bytes per pixel: what GUI toolkits and screen capture hold.  Rows of w * 4 bytes, no
 *                                      constraint on w or h.  X is never used: no result of any entry depends on the fourth byte.
 *                                      For these three the GPU picks the R, G or B byte where it fetches the pixel (csrc/letterbox.hpp,
 *                                      LbPacked), and every result of every entry is bit-identical to the RGB24 entry fed the same pixels
 *                                      with the bytes reordered; y2h_packed_to_rgb24 in libyolo2_host.so restates the reorder.
 * A call is one format.  An odd YUYV / NV12 / I420 width, an odd NV12 / I420 height or an unknown pixfmt is YOLO2_ERROR
 * (yolo2_hip_last_error names it) before anything is launched; yolo2_hip_letterbox_pix also wants a YUYV image_dev on a 4-byte
 * boundary, and an RGBA32 / BGRA32 one likewise (NV12, I420 and BGR24 frames may start at any address).  After a YUYV call yolo2_hip_images_layer0_kernel reports
 * k_conv0_pool_mfma_yuyv[<split>], or under f16_no_mfma0 "k_letterbox_yuyv_batch + " and the frame path's layer-0 kernel; after an
 * NV12 / I420 / BGR24 / RGBA32 / BGRA32 call the same names with _nv12 / _i420 / _bgr24 / _rgba32 / _bgra32. */
enum {
    YOLO2_PIX_GREY8 = 1,
    YOLO2_PIX_RGB24 = 3,
    YOLO2_PIX_YUYV = 0x56595559, /* V4L2 fourcc 'YUYV' */
    YOLO2_PIX_NV12 = 0x3231564E, /* V4L2 fourcc 'NV12' */
    YOLO2_PIX_I420 = 0x32315559, /* V4L2 fourcc 'YU12' = ffmpeg yuv420p */
    YOLO2_PIX_BGR24 = 0x33524742,  /* V4L2 fourcc 'BGR3' = ffmpeg bgr24 */
    YOLO2_PIX_RGBA32 = 0x34324241, /* V4L2 fourcc 'AB24' = ffmpeg rgba (rgb0) */
    YOLO2_PIX_BGRA32 = 0x34325241  /* V4L2 fourcc 'AR24' = ffmpeg bgra (bgr0) */
};
int yolo2_hip_letterbox_pix(uint64_t image_dev, int w, int h, int pixfmt, uint64_t frame_dev, int net_w, int net_h, void *stream);
int yolo2_hip_run_images_pix_host(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                  int pixfmt, int n, int batch, int16_t *region_host, int *final_q);
int yolo2_hip_run_images_pix_dets(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                  int pixfmt, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                  int cap_per_frame, int *counts, int *final_q);
int yolo2_hip_run_images_pix_f16_host(yolo2_hip_ctx *ctx, int split, const uint8_t *const *images, const int *widths,
                                      const int *heights, int pixfmt, int n, int batch, float *region_host);
int yolo2_hip_run_images_pix_dets_f16(yolo2_hip_ctx *ctx, int split, const uint8_t *const *images, const int *widths,
                                      const int *heights, int pixfmt, int n, int batch, float thresh, float nms, int flags,
                                      yolo2_hip_det *dets, int cap_per_frame, int *counts);

/* ------------------------------------------------------- annotated frames: the records painted into the frames they came from
 *
 * The reference's camera / video loop ends every frame with yolo2_draw_detections_rgb24 (linux_app/src/yolo2_draw.c:276-369, called at
 * linux_app/src/main.c:1079-1091) and hands the RGB24 frame to --save-annotated-dir or the MJPEG streamer.  These entries make that
 * frame on the GPU, bit-identical, from the frame in its camera format (YOLO2_PIX_*: RGB24 copied, GREY8 replicated, YUYV / NV12 /
 * I420 converted as above, BGR24 / RGBA32 / BGRA32 reordered) and records of the YOLO2_DETS_BEST_CLASS form (one per detection), whichever pass produced them; no weights are needed.
 *   which records   in array order, those with prob > thresh (and cls >= 0); later records paint over earlier ones
 *   box             corners (int)((x -+ w * 0.5f) * width) etc. in fp32, NaN / out-of-int-range products -> INT_MIN, each clamped to
 *                   the image; 2 pixels thick, every ring clamped again (yolo2_draw_rect_rgb24, :94-111); colour palette[cls % 8]
 *   tag             "<label> <prob %.2f>", at most 127 characters, label = labels[cls] or "class<cls>" (labels NULL, cls >= n_labels, labels[cls] NULL);
 *                   5x7 font at scale 2 (a-z, A-Z as lower case, digits, '.'; anything else a blank that still takes its cell),
 *                   black text on a bright tag (r + g + b > 382), white otherwise; the tag's top is y0 - 18, or y0 + 1 if that is
 *                   negative; rectangle and glyph pixels are cut at the image's edges
 * y2h_draw_detections_rgb24 (libyolo2_host.so) is the same on the host.  Bad arguments - a null pointer, an odd YUYV width, an
 * unknown pixfmt, thresh < 0, a non-positive size, a non-finite prob among the records to be used - are YOLO2_ERROR
 * (yolo2_hip_last_error names the cause) before anything is launched. */

/* One image already on the calling thread's device (the analogue of yolo2_hip_letterbox_pix): image_dev in `pixfmt` (YUYV on a
 * 4-byte boundary) -> rgb_out_dev, w * h * 3 bytes.  dets are n_dets HOST records (NULL if n_dets is 0), labels may be NULL, *drawn
 * (may be NULL) = the records drawn.  Enqueues on `stream` and synchronises it. */
int yolo2_hip_annotate_pix(uint64_t image_dev, int w, int h, int pixfmt, const yolo2_hip_det *dets, int n_dets, float thresh,
                           const char *const *labels, int n_labels, uint64_t rgb_out_dev, int *drawn, void *stream);
/* n images as HOST bytes with the records a yolo2_hip_run_images_*_dets* call returned for them: images / widths / heights / pixfmt
 * and dets [n][cap_per_frame] / counts [n] exactly as that call took and filled them; frame f uses min(counts[f], cap_per_frame)
 * records.  annotated[f] receives w * h * 3 bytes; drawn [n] may be NULL.  Chunks of `batch` (at most 1024); upload, kernel and
 * download of consecutive chunks overlap on three streams through pinned staging the context keeps.  Synchronous. */
int yolo2_hip_annotate_images_pix_host(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                       int pixfmt, int n, int batch, const yolo2_hip_det *dets, int cap_per_frame, const int *counts,
                                       float thresh, const char *const *labels, int n_labels, uint8_t *const *annotated, int *drawn);

/* ------------------------------------------------------- annotated frames as JPEG: the stream of the reference's MJPEG streamer
 *
 * The reference's camera loop hands the annotated frame to its MJPEG streamer, which encodes it with stb_image_write v1.09
 * (stbi_write_jpg_to_func with 3 components, linux_app/src/yolo2_mjpeg_server.c:221-238; quality clamped to 1..100, default 80,
 * main.c:80).  These entries make that stream on the GPU, byte for byte, from RGB24 frames that stay in device memory: baseline JPEG,
 * Y / Cb / Cr without subsampling (one 8x8 block each per MCU, edge pixels repeated), float AAN transform, the typical Huffman
 * tables, no restart markers, a 607-byte header.  Eight launches (csrc/kernels_jpeg.hpp): transform; bit lengths and a two-level
 * scan; code words; 0xFF counts, their scan, and the stuffed stream.  y2h_write_jpg_rgb24 (libyolo2_host.so) is the same encoder
 * on the host.  Width and height are 1..65535, and a frame's bound stays below 2^31 bytes; anything else is YOLO2_ERROR. */

/* The most bytes the stream of a w x h frame can take (607 + twice the scan's bound of 1660 bits per block + 2); 0 for a size these
 * entries refuse (outside 1..65535, or a bound of 2^31 bytes or more). */
size_t yolo2_hip_jpeg_bound(int w, int h);
/* One RGB24 frame already on the calling thread's device -> its stream at jpeg_out_dev; neither address needs any alignment.
 * *size = the stream's length.  If it exceeds cap, nothing at or beyond cap is written and the call returns YOLO2_ERROR ("too
 * small"; *size is still set, jpeg_out_dev may be 0 if cap is 0).  Enqueues on `stream` and synchronises it. */
int yolo2_hip_jpeg_encode_rgb24(uint64_t rgb_dev, int w, int h, int quality, uint64_t jpeg_out_dev, size_t cap, size_t *size, void *stream);
/* yolo2_hip_annotate_images_pix_host with JPEG streams out: the painter writes RGB24 into device memory, the encoder follows on the
 * same stream, and the frame never visits the host.  jpeg[f] has room for caps[f] bytes and receives min(sizes[f], caps[f]); the
 * download copies the sizes first and then only the bytes in use.  A frame whose stream exceeds its capacity gets its sizes[f]
 * and nothing past the capacity, the other frames are complete, and the call returns YOLO2_ERROR ("too small").  A frame without
 * records in YOLO2_PIX_RGB24 is a pure encode.  drawn [n] may be NULL.  Synchronous. */
int yolo2_hip_annotate_images_pix_jpeg_host(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                            int pixfmt, int n, int batch, const yolo2_hip_det *dets, int cap_per_frame, const int *counts,
                                            float thresh, const char *const *labels, int n_labels, int quality, uint8_t *const *jpeg,
                                            const size_t *caps, size_t *sizes, int *drawn);

/* ------------------------------------------------------- the camera loop as one call
 *
 * What yolo2_linux produces per frame (linux_app/src/main.c:942-1091) - the detection records and the annotated frame - from one
 * upload: per chunk the frames are staged once and go up in one H2D, the network of the chosen precision reads them from the chunk's
 * device staging buffer (the path of yolo2_hip_run_images_pix_dets[_f16]), the tail leaves its records in HBM, k_draw_items turns them
 * into the painter's draw items on the device (corner casts, rings, tag and the "%s %.2f" text in integers: csrc/draw_list.hpp),
 * k_annotate_batch paints from the SAME staging buffer, and with YOLO2_LOOP_OUT_JPEG the encoder follows.  Counts, records and the
 * frames (or the sizes and only the stream bytes in use) come back.
 *
 * dets / counts / final_q (int16 only; may be NULL) are exactly what yolo2_hip_run_images_pix_dets (YOLO2_LOOP_INT16) or
 * yolo2_hip_run_images_pix_dets_f16 (split 0: YOLO2_LOOP_FP16, split 1: YOLO2_LOOP_F32TOL) return for the same arguments.  flags must
 * contain YOLO2_DETS_BEST_CLASS (the form the painter draws; YOLO2_DETS_APP_TAIL selects the camera loop's tail); one thresh serves the
 * records and the painter (main.c:1081).  out[f] (caps[f] bytes of room) and sizes[f]: with YOLO2_LOOP_OUT_RGB24 the bytes
 * yolo2_hip_annotate_images_pix_host writes for those records, sizes[f] = w * h * 3, and a caps[f] below that is refused up front;
 * with YOLO2_LOOP_OUT_JPEG (quality 1..100) the semantics of yolo2_hip_annotate_images_pix_jpeg_host; with YOLO2_LOOP_OUT_BGR24 the
 * YOLO2_LOOP_OUT_RGB24 frame with bytes 0 and 2 of every pixel exchanged (what cv2.imshow / cv2.VideoWriter take; k_annotate_batch_bgr),
 * same sizes and capacities, from any source format, quality ignored.  drawn [n] may be NULL.
 * With YOLO2_LOOP_OUT_NV12 / YOLO2_LOOP_OUT_I420 the YOLO2_LOOP_OUT_RGB24 frame comes back as planar YUV 4:2:0, what video encoders take
 * (ffmpeg -f rawvideo -pix_fmt nv12 | yuv420p), in the layout of YOLO2_PIX_NV12 / YOLO2_PIX_I420: Y [h][w], then NV12's interleaved U V
 * rows [h/2][w] or I420's U [h/2][w/2] and V [h/2][w/2]; sizes[f] = w * h * 3 / 2 (half of RGB24's bytes over PCIe), a caps[f] below that
 * is refused up front, and so is an odd width or height (before any launch and any write to the caller's arrays), quality ignored.
 * The conversion is the library's own definition, in integers (>> arithmetic, no clamp needed: Y 16..235, U and V 16..240):
 *   per pixel        Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
 *   per 2x2 block    U = ((-38 Rs - 74 Gs + 112 Bs + 512) >> 10) + 128,  V = ((112 Rs - 94 Gs - 18 Bs + 512) >> 10) + 128
 * with Rs, Gs, Bs the sums of the block's four pixels (chroma of the block's mean colour).  It is the BT.601 studio-range forward
 * transform whose constants pair with the inverse the 4:2:0 and YUYV inputs use (298 / 409 / 100 / 208 / 516); the reference has no
 * YUV output, and identity with swscale's YUV is not claimed.  y2h_rgb24_to_yuv420 in libyolo2_host.so restates it on the host
 * (k_annotate_batch_nv12 / _i420 compute it where the painter stores).  Everything else is what the call returns for RGB24 out.
 * A record that would be drawn but whose prob is not finite (or is 2^23 and more) is not drawn; the call then returns YOLO2_ERROR
 * naming the first such frame, everything else is complete.  Refused before any launch: what the entries it joins refuse.
 * Synchronous; batch <= 1024, cap_per_frame <= 65536. */
enum { YOLO2_LOOP_INT16 = 0, YOLO2_LOOP_FP16 = 1, YOLO2_LOOP_F32TOL = 2 };
enum { YOLO2_LOOP_OUT_RGB24 = 0, YOLO2_LOOP_OUT_JPEG = 1, YOLO2_LOOP_OUT_BGR24 = 0x33524742 /* V4L2 fourcc 'BGR3' */,
       YOLO2_LOOP_OUT_NV12 = 0x3231564E /* 'NV12' */, YOLO2_LOOP_OUT_I420 = 0x32315559 /* 'YU12' */ };
int yolo2_hip_loop_images_pix(yolo2_hip_ctx *ctx, int precision, const uint8_t *const *images, const int *widths, const int *heights,
                              int pixfmt, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap_per_frame,
                              int *counts, int *final_q, const char *const *labels, int n_labels, int out_format, int quality,
                              uint8_t *const *out, const size_t *caps, size_t *sizes, int *drawn);
/* What the last loop call on this context moved and built. */
typedef struct {
    int chunks;
    uint64_t image_bytes_staged;   /* frame bytes copied into pinned staging (each frame once) */
    uint64_t image_bytes_h2d;      /* bytes of the chunks' uploads: the letterbox and painter tables, then the padded frames */
    uint64_t out_bytes_d2h;        /* painted frames, or sizes and stream bytes, that came back (records and counts not included) */
    uint64_t items_built;          /* drawn records, as counted on the device */
    char items_kernel[32];         /* "k_draw_items" */
} yolo2_hip_loop_info_t;
int yolo2_hip_loop_last_info(yolo2_hip_ctx *ctx, yolo2_hip_loop_info_t *info);
/* Test doorway to k_draw_items: records [n_frames][cap_per_frame] and counts [n_frames] ON THE DEVICE -> the items it makes of them
 * (frame f's at items + f * cap_per_frame * yolo2_hip_draw_item_size(), n_items[f] of them, in record order), as RGB24 frames of
 * widths x heights would have them.  unprintable [n_frames] (may be NULL): the drawn records left out for their prob; any such
 * record makes the call YOLO2_ERROR naming the first such frame, with all outputs complete. */
size_t yolo2_hip_draw_item_size(void);
int yolo2_hip_draw_items_dev(yolo2_hip_ctx *ctx, uint64_t dets_dev, uint64_t counts_dev, int n_frames, int cap_per_frame, const int *widths,
                             const int *heights, float thresh, const char *const *labels, int n_labels, void *items, int *n_items,
                             int *unprintable);

/* ------------------------------------------------------- calibration: fp32 weights + frames -> int16 weights and Q tables
 *
 * The reference makes its int16 weight set with a separate tool (weights/README.md step 2b: "activation-calibrated"
 * weight_int16.bin, bias_int16.bin, weight_int16_Q.bin, bias_int16_Q.bin, iofm_Q.bin).  These entries are that step on the GPU, from what
 * yolo2_hip_load_weights_fp32 left resident: the exact fp32 pass (bit-identical to the reference's fp32) runs the calibration frames
 * and one abs-max reduction per tensor gives the range of the input and of every conv layer's unpooled output.
 *
 * Q rule: q(m, h) = the largest integer q in 0..15 at which h * m still quantises to at most 32767, i.e. h * m * 2^q < 32767.5
 * (rounding is half away from zero), in double; m = 0 gives 15; no such q is YOLO2_ERROR naming the tensor.  So 1.0 -> 14,
 * 3.9999 -> 13 (32767.18 rounds to 32767), 4.0 -> 12, 32767 -> 0, 32768 -> error.  weight_q[ord] = q(max |w_ord|, 1), bias_q[ord] = q(max |b_ord|, 1), act_q[0] = q(max |input|, 1) (frames in
 * [0, 1] give 14), act_q[ord + 1] = q(max |out_ord|, headroom) with the caller's headroom >= 1.  One fix-up: the layer loop
 * (yolo2_model.cpp:379-399) only shifts the reorg half of the concat tensor DOWN to layer 24's Q, so if layer 24's output Q came out
 * above layer 26's it is lowered to layer 26's.
 *
 * Every entry refuses bad arguments before anything is launched; yolo2_hip_last_error names the cause. */

/* max |x| over n floats in HBM (any 4-byte-aligned address), and the number of Inf / NaN among them - counted, and left out of the
 * maximum (the count saturates: exact below 2^20 per workgroup of the reduction).  On the calling thread's current device;
 * synchronises `stream`.  nonfinite may be NULL. */
int yolo2_hip_absmax_f32(uint64_t data_dev, size_t n, float *absmax, uint32_t *nonfinite, void *stream);
/* Clears the context's statistics (they accumulate over calls).  Call it after loading another weight set. */
int yolo2_hip_calib_reset(yolo2_hip_ctx *ctx);
/* One exact fp32 pass over frames_dev (float [batch][3][416][416], device) and the 24 reductions, accumulated.  Needs
 * yolo2_hip_load_weights_fp32; batch limits are yolo2_hip_run_batch_fp32's.  The frames are looked at first: a NaN or Inf among them
 * is YOLO2_ERROR with nothing accumulated.  Enqueues on `stream` and synchronises it. */
int yolo2_hip_calib_frames(yolo2_hip_ctx *ctx, uint64_t frames_dev, int batch, void *stream);
/* The same from n images as HOST bytes, letterboxed on the GPU in chunks of `batch` (pixfmt: YOLO2_PIX_*). */
int yolo2_hip_calib_images_pix_host(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                    int pixfmt, int n, int batch);
/* act_absmax[24]: the network input, then the output of conv ordinal 0..22; weight_absmax[23] / bias_absmax[23]: the resident fp32
 * blobs per conv ordinal; *frames_seen: frames accumulated since the last reset.  Any of the four may be NULL. */
int yolo2_hip_calib_stats(yolo2_hip_ctx *ctx, float *act_absmax, float *weight_absmax, float *bias_absmax, long *frames_seen);
/* The Q rule above on the context's statistics -> weight_q[23], bias_q[23], act_q[24].  YOLO2_ERROR if no frame was seen or a
 * non-finite value was counted in any tensor. */
int yolo2_hip_calib_q_tables(yolo2_hip_ctx *ctx, float headroom, int32_t *weight_q, int32_t *bias_q, int32_t *act_q);
/* The Q rule on explicit maxima (host arithmetic only, no GPU): act_absmax[24], weight_absmax[23], bias_absmax[23] as above. */
int yolo2_hip_calib_q_from_stats(const float *act_absmax, const float *weight_absmax, const float *bias_absmax, float headroom,
                                 int32_t *weight_q, int32_t *bias_q, int32_t *act_q);
/* int16 = round(x * 2^Q) of the resident fp32 blobs, on the GPU, into host buffers of at least YOLO2_N_WEIGHTS / YOLO2_N_BIAS
 * elements, in the order yolo2_hip_load_weights_int16 takes (on this or another context).  The rule is the network input's
 * (yolo2_model.cpp:257-273): product in fp32, clamped, rounded half away from zero - clamped symmetrically to +-32767.  Any tables
 * with Q in 0..30 may be passed, not only calibrated ones; *clamped (may be NULL) = the values whose rounded product lay outside
 * +-32767 (|x * 2^Q| >= 32767.5; a NaN counts and becomes 0). */
int yolo2_hip_quantize_weights_int16(yolo2_hip_ctx *ctx, const int32_t *weight_q, const int32_t *bias_q, int16_t *weights_reorg_out,
                                     size_t n_weights, int16_t *bias_out, size_t n_bias, long *clamped);

/* ------------------------------------------------------- int8 pass: calibrate, quantise and run on the i8 matrix cores
 *
 * A quantised integer pass of this project's own definition (the reference has no int8 mode): int8 activations and weights, exact
 * int32 accumulation on v_mfma_i32_32x32x32_i8, one requantisation per output.  It is int8-grade (about 10 % region noise on the
 * synthetic model), deterministic and bit-exact against tests/i8ref.py; it replaces neither the int16 nor the fp16 pass.
 *
 * Q rule: q8(m, h) = the largest integer q in -8..24 with h * m * 2^q < 127.5, in double; m = 0 gives 24; no such q is YOLO2_ERROR
 * naming the tensor.  Qw[o][m] = q8(max |w| of output channel m of conv o, 1); act_q[0] = q8(max |input|, 1) (frames in [0, 1]
 * give 6); act_q[o + 1] = q8(max |out_o|, headroom).  Fix-up: act_q[20] (layer 24) and act_q[21] (layer 26) are both set to the
 * smaller of the two, so the concat tensor layer 29 reads has one Q.  Qin(o), the Q of the tensor conv o reads, is act_q[o], except
 * act_q[13] for layer 26 (route 25) and act_q[20] for layer 29.
 * Quantise: w8 = clamp(round_half_away(w * 2^Qw), -127, 127); bias32 = round_half_away(b * 2^(Qin + Qw)) in double;
 * input x8 = clamp(round_half_away(x * 2^act_q[0]), -128, 127).
 * Conv: acc = bias32 + sum(w8 * x8) in int32 with zero padding; leaky: acc < 0 -> acc / 10 truncating toward zero;
 * s = Qin + Qw - act_q[o + 1]; y = (acc + 2^(s-1)) >> s for s > 0, acc << -s (64 bits) otherwise; out = clamp(y, -128, 127).
 * Pool is a 2x2 max, reorg the legacy Darknet indexing, route is placement.  Layer 30 is not requantised:
 * region = (float)acc * 2^-(Qin + Qw), round-to-nearest conversion and an exact scaling.
 * Entries: frames in HBM (yolo2_hip_run_batch_int8) and image bytes on the host (yolo2_hip_run_images_pix_int8_host / _dets_int8,
 * below).  The loop and multi-GPU entries have no int8 form. */

/* The int8 Q rule on explicit maxima (host arithmetic only, no GPU): act_absmax[24] as yolo2_hip_calib_stats returns them ->
 * act_q[24], fix-up applied. */
int yolo2_hip_calib_q8_from_stats(const float *act_absmax, float headroom, int32_t *act_q);
/* The same on the context's statistics.  YOLO2_ERROR if no frame was seen or a non-finite value was counted in a tensor. */
int yolo2_hip_calib_q8_tables(yolo2_hip_ctx *ctx, float headroom, int32_t *act_q);
/* The resident fp32 blobs quantised on the GPU (k_quantize_i8: per-channel abs-max, then w8, bias32 and Qw) into host buffers:
 * w8_out, at least YOLO2_N_WEIGHTS int8 in NATURAL [N][C][K][K] order per layer; bias32_out and weight_q_out, at least YOLO2_N_BIAS
 * each, one entry per output channel.  act_q[24] supplies Qin of every layer.  A channel that no Q holds is YOLO2_ERROR naming it. */
int yolo2_hip_quantize_weights_int8(yolo2_hip_ctx *ctx, const int32_t *act_q, int8_t *w8_out, size_t n_w, int32_t *bias32_out, size_t n_b,
                                    int32_t *weight_q_out);
/* Loads an int8 weight set (host arrays as the quantiser writes them; n_w = YOLO2_N_WEIGHTS, n_b = YOLO2_N_BIAS, weight_q[n_b],
 * act_q[24]) and packs the weights on the device in the order the conv kernel stages them.  Refused before any launch: wrong
 * lengths; a Q outside -8..24; act_q[20] != act_q[21]; a shift s outside -7..31; an output channel for which
 * |bias32| + 128 * sum|w8| + 2^30 < 2^31 does not hold (the proof that neither the accumulator nor its rounding constant can
 * overflow 32 bits) - the message names the layer and the channel.  Independent of the int16 and fp32 weight sets of the context. */
int yolo2_hip_load_weights_int8(yolo2_hip_ctx *ctx, const int8_t *w8, size_t n_w, const int32_t *bias32, size_t n_b, const int32_t *weight_q,
                                const int32_t *act_q);
/* The int8 pass: frames_dev float [batch][3][416][416] -> region_dev float [batch][425][13][13], both in HBM and laid out as
 * yolo2_hip_run_batch_fp16 has them; the region tensor feeds yolo2_hip_postprocess_f32 / _f32_app.  One stream, no lanes; enqueues
 * and returns.  batch 1..1024. */
int yolo2_hip_run_batch_int8(yolo2_hip_ctx *ctx, uint64_t frames_dev, int batch, uint64_t region_dev, void *stream);
/* The same with host buffers, blocking. */
int yolo2_hip_run_batch_int8_host(yolo2_hip_ctx *ctx, const float *frames, int batch, float *region);
/* Image bytes to region tensors / detection records on the int8 pass, single device: the contract of
 * yolo2_hip_run_images_pix_f16_host / _dets_f16 (chunks of `batch` images, 1..1024, a ragged last chunk repeats its last image;
 * staging, upload, kernels and download overlap on the context's three streams; region_host float [n][425][13][13]; the records
 * come from the float tail, flags YOLO2_DETS_BEST_CLASS / YOLO2_DETS_APP_TAIL).  pixfmt: any YOLO2_PIX_*.
 * One kernel (k_i8_front_u8 / k_i8_front_yuyv / k_i8_front_nv12 / k_i8_front_i420 / k_i8_front_bgr24 / k_i8_front_rgba32 / k_i8_front_bgra32) goes from the chunk's bytes to layer 1's tensor: letterbox, the input rule above,
 * layer 0 with its 27 inputs in one k step of v_mfma_i32_32x32x32_i8, and the 2x2 pool.  The result equals, bit for bit, the chunk
 * letterboxed (yolo2_hip_letterbox_pix) and run through yolo2_hip_run_batch_int8, which is what the entries do under option
 * i8_no_front.  The quantised input and layer 0's tensor (2 * batch * 416 * 416 * 32 bytes) are not allocated on this route.
 * Refused before any launch: int8 weights not loaded, a null pointer or image, n, batch or cap_per_frame <= 0, thresh < 0, an
 * unknown pixfmt, an odd YUYV width, an image size the letterbox refuses. */
int yolo2_hip_run_images_pix_int8_host(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                       int pixfmt, int n, int batch, float *region_host);
int yolo2_hip_run_images_pix_dets_int8(yolo2_hip_ctx *ctx, const uint8_t *const *images, const int *widths, const int *heights,
                                       int pixfmt, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                       int cap_per_frame, int *counts);
/* What the last int8 images call on ctx ran up to layer 1: "k_i8_front_u8", "k_i8_front_yuyv", "k_i8_front_nv12", "k_i8_front_i420", "k_i8_front_bgr24", "k_i8_front_rgba32" or "k_i8_front_bgra32"; under i8_no_front
 * "k_letterbox_u8_batch + k_i8_quant_input + k_conv_i8" (or k_letterbox_yuyv_batch ...); "" before the first call. */
const char *yolo2_hip_images_front_kernel_int8(yolo2_hip_ctx *ctx);
/* Parity hook: the int8 tensor layer `layer_idx` (0..29; -1 = the quantised input) left behind in the last int8 run, frame `frame`,
 * as dense [C][H][W] into out (cap elements).  geom[4] = {C, H, W, Q}; out may be NULL to ask for the geometry only.  Locates a
 * wrong layer without another run.  After an images call it reads the call's last chunk (frame: the index inside that chunk); the
 * fused front kernel writes neither the quantised input nor layer 0, so layers -1 and 0 are then YOLO2_ERROR ("fused"); under
 * i8_no_front and after a frames run they are readable. */
int yolo2_hip_debug_i8_tensor(yolo2_hip_ctx *ctx, int layer_idx, int frame, int8_t *out, size_t cap, int *geom);
/* Driver-tier single layer beside yolo2_execute_conv_layer / _f32: one stride-1 "same" conv of any ifm_num, ofm_num, ksize 1 or 3,
 * size and batch through the int8 kernel.  Device buffers in natural dense order: input int8 [batch][ifm][H][W], weights int8
 * [ofm][ifm][k][k], bias32 int32 [ofm], output int8 [batch][ofm][H][W] or - out_float - float of the same shape computed by layer
 * 30's rule.  weight_q[ofm] is a HOST array.  The loader's refusals (Q ranges, s, the overflow proof) apply.  Blocking. */
int yolo2_execute_conv_layer_int8(uint64_t input_addr, uint64_t output_addr, uint64_t weight_addr, uint64_t bias_addr,
                                  const int32_t *weight_q, int ifm_num, int ofm_num, int ksize, int input_w, int input_h, int batch,
                                  int q_in, int q_out, int is_nl, int out_float, uint32_t timeout_ms);

/* ------------------------------------------------------- JPEG streams decoded on the GPU
 *
 * The reference's camera loop asks the camera for MJPEG first (linux_app/src/yolo2_v4l2.c:112-123) and its image path opens JPEG
 * files; these entries take the compressed streams.  The host reads the headers only; Huffman decode, inverse DCT, up-sampling and
 * colour conversion run on the device (k_jpegdec_entropy, one lane per restart interval; k_jpegdec_idct; k_jpegdec_rgb) and leave
 * RGB24 in the chunk staging layout the images entries read, so the network's kernels run unchanged behind them.  The bytes are
 * those of the host decoder (host/y2_codec.cpp, and so stb_image's) on every stream the decoder accepts.
 *
 * GPU-decodable: SOF0 / SOF1, 8-bit, Huffman; 1 component, or 3 components YCbCr (not the R,G,B component ids, not Adobe
 * transform 0 without JFIF) with chroma sampling 1x1 and luma H, V each 1 or 2; exactly one scan holding all components; every
 * Huffman table the scan names defined; any restart interval or none; EOI behind the scan; at most 16384 in a direction and 2^26
 * pixels.  Everything else has a reason code and goes through the host decoder as before.
 *
 * Per-frame status (YOLO2_JPEG_ST_*): 0; a bad Huffman code; a coefficient index past 63; "restart out of step" - a restart interval
 * that did not end at its marker, a count of RSTn markers that does not fit the geometry, or a last interval that does not end at
 * the marker closing the scan: every case in which the host decoder's result depends on state carried across intervals.  Where
 * several intervals of a frame fail, the first in stream order gives the status.  A flagged frame is not a guess: its pixels are
 * zero-filled and the caller decodes it on the host.
 *
 * Out of scope here (they keep taking raw frames): the annotate-only entries, the calibration entry and bench.py; the colour stage
 * is not fused into the letterbox or layer-0 kernels.  The loop entry from streams is yolo2_hip_loop_images_jpeg below, the
 * multi-GPU forms are in the multi-GPU section. */
enum {
    YOLO2_JPEG_OK = 0, YOLO2_JPEG_DAMAGED = 1, YOLO2_JPEG_PROGRESSIVE = 2, YOLO2_JPEG_UNSUPPORTED_SOF = 3, YOLO2_JPEG_COMPONENTS = 4,
    YOLO2_JPEG_RGB_COLOUR = 5, YOLO2_JPEG_SAMPLING = 6, YOLO2_JPEG_SCANS = 7, YOLO2_JPEG_MISSING_TABLE = 8, YOLO2_JPEG_TOO_LARGE = 9
};
enum { YOLO2_JPEG_ST_OK = 0, YOLO2_JPEG_ST_BAD_CODE = 1, YOLO2_JPEG_ST_COEF_OVERRUN = 2, YOLO2_JPEG_ST_RESTART = 3 };
typedef struct {
    int width, height, components, hmax, vmax, restart_interval;
    int gpu_decodable, reason;   /* reason: YOLO2_JPEG_* (0 iff gpu_decodable) */
    size_t stream_bytes;         /* offset just past EOI, or size: cuts a concatenated MJPEG stream */
} yolo2_hip_jpeg_info_t;
/* Host only, no GPU call.  The segments are walked by their lengths; inside a scan the end is FF followed by anything but 00, FF or
 * D0..D7.  Returns YOLO2_SUCCESS whatever the class (YOLO2_ERROR: null argument). */
int yolo2_hip_jpeg_probe(const uint8_t *jpeg, size_t size, yolo2_hip_jpeg_info_t *info);
const char *yolo2_hip_jpeg_reason_name(int reason);
/* n streams -> RGB24 in host memory (rgb_out[i], caps[i] bytes of room), in chunks of `batch`; widths / heights / status [n] are
 * filled.  Refused before any launch, naming the first frame and the probe's reason: a stream the probe does not accept, a caps[i]
 * below w * h * 3.  A frame whose status is not 0 is zero-filled and the call returns YOLO2_ERROR naming the first such frame, every
 * other frame complete.  No weights are needed. */
int yolo2_hip_decode_jpeg_host(yolo2_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, int n, int batch,
                               uint8_t *const *rgb_out, const size_t *caps, int *widths, int *heights, int *status);
/* The same functions (csrc/jpeg_scan.hpp) run on the host, one frame, no GPU call: the doorway of the CPU tests and of
 * tools/fuzz_jpegdec.cpp.  A stream the probe refuses: YOLO2_ERROR, *status = 100 + reason. */
int yolo2_hip_decode_jpeg_ref(const uint8_t *stream, size_t size, uint8_t *rgb_out, size_t cap, int *width, int *height, int *status);
/* Streams -> detection records: yolo2_hip_run_images_pix_dets (precision YOLO2_LOOP_INT16), _pix_dets_f16 (split 0: _FP16, split 1:
 * _F32TOL) or _pix_dets_int8 (YOLO2_JPEG_INT8) fed the decoded RGB24 frames - the same kernels read the same bytes, so counts,
 * records and final_q (int16 only; may be NULL) are identical.  sizes[i] == 0: frame i is raw RGB24 of widths[i] x heights[i] at
 * streams[i], copied to its slot as in those entries (a caller mixes host-decoded frames into a chunk); for the others widths /
 * heights are filled from the headers.  Refusals as above plus the joined entry's.  A frame whose status is not 0: zero-filled
 * before the network reads it, counts[f] = 0, and the call returns YOLO2_ERROR naming the first such frame with every other frame
 * complete (the loop entry's rule for unprintable records).  status [n] may not be NULL. */
#define YOLO2_JPEG_INT8 3
int yolo2_hip_run_images_jpeg_dets(yolo2_hip_ctx *ctx, int precision, const uint8_t *const *streams, const size_t *sizes,
                                   int *widths, int *heights, int n, int batch, float thresh, float nms, int flags,
                                   yolo2_hip_det *dets, int cap_per_frame, int *counts, int *final_q, int *status);
/* Of the last of the two calls above on ctx, for reports: out8[0..3] device-event milliseconds per chunk (mean over the call's
 * chunks) of the coefficient memset, k_jpegdec_entropy, k_jpegdec_idct and k_jpegdec_rgb (+ k_jpegdec_zero) - zero unless
 * yolo2_hip_set_profiling was on -; [4] bytes uploaded as descriptors, tables and streams; [5] bytes uploaded as letterbox tables
 * and raw frames; [6] chunks; [7] frames. */
int yolo2_hip_jpeg_last_info(yolo2_hip_ctx *ctx, double *out8);
/* Option "jpegdec_split" = S (yolo2_hip_set_option; a multiple of 16 in 16..4096, read per call, 0 / unset: the launches above
 * exactly): the entropy stage gives a segment one lane per S raw bytes instead of one lane (k_jpegdec_split).  S is
 * doubled for a segment until at most 2048 subsequences cover it; a segment shorter than two subsequences keeps its one lane.  The
 * split lanes' result is accepted only where it is provably the one lane's; every other segment is decoded by the one-lane function
 * in the same call (k_jpegdec_rest), so status words and bytes are those of the call without the option, always.
 * yolo2_hip_jpeg_last_info's entropy figure is then the sum over the stage's launches.
 * The doorway: yolo2_hip_decode_jpeg_ref with the entropy stage run that way on the host, lanes and rounds as loops, no GPU call;
 * info8 as out8[0..5] below. */
int yolo2_hip_decode_jpeg_split_ref(const uint8_t *stream, size_t size, int split_bytes, uint8_t *rgb_out, size_t cap, int *width,
                                    int *height, int *status, double *info8);
/* Of the last JPEG call on ctx (all zero when the option was unset): out8[0] subsequences, [1] segments split-decoded, [2] segments
 * that fell back to the one-lane function, [3] segments too short to split, [4] most synchronisation rounds of any segment, [5] S,
 * [6] / [7] device-event milliseconds per chunk of k_jpegdec_split and of k_jpegdec_rest (under yolo2_hip_set_profiling). */
int yolo2_hip_jpeg_split_info(yolo2_hip_ctx *ctx, double *out8);
/* The camera loop as one call FROM STREAMS: yolo2_hip_loop_images_pix (YOLO2_PIX_RGB24) with the decoder above in front of it, the
 * decoded frame never leaving the device.  The decoder kernels write each frame into the slot of the chunk's staging buffer that the
 * network's front kernel, k_draw_items' painter k_annotate_batch and the encoder then read, so dets, counts, final_q, drawn, out[f]
 * and out_sizes[f] are, byte for byte, what yolo2_hip_decode_jpeg_host followed by yolo2_hip_loop_images_pix on its frames returns;
 * only compressed bytes, tables and records cross PCIe in either direction (with YOLO2_LOOP_OUT_RGB24 the painted frames come back).
 * Arguments as yolo2_hip_run_images_jpeg_dets (streams, sizes, widths, heights - sizes[i] == 0: frame i is raw RGB24 of widths[i] x
 * heights[i] - and status [n], which may not be NULL) and as yolo2_hip_loop_images_pix (everything else; out_sizes is its `sizes`).
 * precision: YOLO2_LOOP_INT16, _FP16 or _F32TOL; YOLO2_JPEG_INT8 is refused (the loop entries have no int8 form).  flags must
 * contain YOLO2_DETS_BEST_CLASS; YOLO2_DETS_APP_TAIL is honoured.  Option jpegdec_split is read per call.
 * Refused before any launch, every output (widths / heights included) untouched: what the probe refuses, with its reason; what
 * yolo2_hip_loop_images_pix and yolo2_hip_run_images_jpeg_dets refuse; with YOLO2_LOOP_OUT_RGB24 a caps[f] below w * h * 3 of the
 * header; with YOLO2_LOOP_OUT_NV12 / _I420 a header whose width or height is odd, or a caps[f] below w * h * 3 / 2.  A frame whose scan the decoder flags: status[f] != 0, counts[f] = 0, drawn[f] = 0, out_sizes[f] = 0, nothing is written
 * to out[f], and the call returns YOLO2_ERROR naming the first such frame with every other frame complete.
 * Afterwards yolo2_hip_jpeg_last_info, _jpeg_split_info and _loop_last_info describe the call: image_bytes_staged is stream bytes plus
 * raw-frame bytes, image_bytes_h2d everything uploaded (blobs, tables, raw frames); jpeg_last_info [5] counts the painter's and the
 * encoder's tables with the letterbox tables. */
int yolo2_hip_loop_images_jpeg(yolo2_hip_ctx *ctx, int precision, const uint8_t *const *streams, const size_t *sizes, int *widths,
                               int *heights, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                               int cap_per_frame, int *counts, int *final_q, const char *const *labels, int n_labels, int out_format,
                               int quality, uint8_t *const *out, const size_t *caps, size_t *out_sizes, int *drawn, int *status);

/* ------------------------------------------------------- multi-GPU: frame sharding, one weight broadcast
 *
 * SURVEY.md 8(b) "init(device_list) ... load_weights (H2D on rank 0, RCCL broadcast to the rest)", 8(e): frames are
 * independent, so every GPU holds the whole weight set, frames split into contiguous ranges, and the only collective is
 * ONE broadcast of the weight blobs at init (ncclBroadcast from librccl.so, RCCL over xGMI; the library is loaded at the
 * first call of this section, single-GPU users never load it).  Both launch models share that one broadcast routine. */

/* contiguous range [lo, hi) of `rank` among `world` shards of `total` frames; sizes differ by at most one */
int yolo2_hip_shard_range(int total, int rank, int world, int *lo, int *hi);

/* (a) one process, n devices - the C host's model (yolov2_detect --devices 0,1,...): one context per device, a RCCL
 * communicator over the list (ncclCommInitAll).  A list that names one device twice rehearses the sharding on a single
 * GPU: RCCL refuses duplicate devices, so such a list copies device-to-device instead (yolo2_hip_multi_uses_rccl = 0). */
typedef struct yolo2_hip_multi yolo2_hip_multi;
int  yolo2_hip_multi_create(const int *devices, int n_devices, yolo2_hip_multi **m);
void yolo2_hip_multi_destroy(yolo2_hip_multi *m);
int  yolo2_hip_multi_num_devices(yolo2_hip_multi *m);
int  yolo2_hip_multi_uses_rccl(yolo2_hip_multi *m);
yolo2_hip_ctx *yolo2_hip_multi_ctx(yolo2_hip_multi *m, int i);      /* borrowed: for set_batch / profiling / layer_path */
/* blobs: host -> devices[0] -> ncclBroadcast to the rest -> every context loads its device copy */
int  yolo2_hip_multi_load_weights_int16(yolo2_hip_multi *m, const int16_t *weights_reorg, size_t n_weights,
                                        const int16_t *bias, size_t n_bias, const int32_t *weight_q, int n_weight_q,
                                        const int32_t *bias_q, int n_bias_q, const int32_t *act_q, int n_act_q);
int  yolo2_hip_multi_load_weights_fp32(yolo2_hip_multi *m, const float *weights_reorg, size_t n_weights,
                                       const float *bias, size_t n_bias);
/* n_frames host frames -> region tensors, shard i streamed by device i (yolo2_hip_run_frames_int16 / _run_images_u8_host
 * on its own host thread, chunks of batch_per_device); no data-path collective.  Results do not depend on the device count. */
int  yolo2_hip_multi_run_frames_int16(yolo2_hip_multi *m, const float *frames, int n_frames, int batch_per_device,
                                      int16_t *region, int *final_q);
int  yolo2_hip_multi_run_images_u8_host(yolo2_hip_multi *m, const uint8_t *const *images, const int *widths,
                                        const int *heights, int channels, int n, int batch_per_device,
                                        int16_t *region_host, int *final_q);

/* images -> detection records, shard i on device i: network AND tail run on the device that owns the shard (no region tensor
 * travels to the host or to device 0); see yolo2_hip_run_images_u8_dets. */
int  yolo2_hip_multi_run_images_u8_dets(yolo2_hip_multi *m, const uint8_t *const *images, const int *widths, const int *heights,
                                        int channels, int n, int batch_per_device, float thresh, float nms, int flags,
                                        yolo2_hip_det *dets, int cap_per_frame, int *counts, int *final_q);
/* the same on the fp16 (split = 0) / fp32-tolerance (split = 1) pass; see yolo2_hip_run_images_u8_dets_f16 */
int  yolo2_hip_multi_run_images_u8_dets_f16(yolo2_hip_multi *m, int split, const uint8_t *const *images, const int *widths,
                                            const int *heights, int channels, int n, int batch_per_device, float thresh, float nms,
                                            int flags, yolo2_hip_det *dets, int cap_per_frame, int *counts);
/* the three with a pixel format (see yolo2_hip_run_images_pix_host) */
int  yolo2_hip_multi_run_images_pix_host(yolo2_hip_multi *m, const uint8_t *const *images, const int *widths,
                                         const int *heights, int pixfmt, int n, int batch_per_device,
                                         int16_t *region_host, int *final_q);
int  yolo2_hip_multi_run_images_pix_dets(yolo2_hip_multi *m, const uint8_t *const *images, const int *widths, const int *heights,
                                         int pixfmt, int n, int batch_per_device, float thresh, float nms, int flags,
                                         yolo2_hip_det *dets, int cap_per_frame, int *counts, int *final_q);
int  yolo2_hip_multi_run_images_pix_dets_f16(yolo2_hip_multi *m, int split, const uint8_t *const *images, const int *widths,
                                             const int *heights, int pixfmt, int n, int batch_per_device, float thresh, float nms,
                                             int flags, yolo2_hip_det *dets, int cap_per_frame, int *counts);

/* annotated frames (see yolo2_hip_annotate_images_pix_host), shard i painted by device i */
int  yolo2_hip_multi_annotate_images_pix_host(yolo2_hip_multi *m, const uint8_t *const *images, const int *widths, const int *heights,
                                              int pixfmt, int n, int batch_per_device, const yolo2_hip_det *dets, int cap_per_frame,
                                              const int *counts, float thresh, const char *const *labels, int n_labels,
                                              uint8_t *const *annotated, int *drawn);

/* annotated frames as JPEG streams (see yolo2_hip_annotate_images_pix_jpeg_host), shard i painted and encoded by device i */
int  yolo2_hip_multi_annotate_images_pix_jpeg_host(yolo2_hip_multi *m, const uint8_t *const *images, const int *widths, const int *heights,
                                                   int pixfmt, int n, int batch_per_device, const yolo2_hip_det *dets, int cap_per_frame,
                                                   const int *counts, float thresh, const char *const *labels, int n_labels, int quality,
                                                   uint8_t *const *jpeg, const size_t *caps, size_t *sizes, int *drawn);

/* the camera loop as one call (see yolo2_hip_loop_images_pix), shard i on device i; yolo2_hip_loop_last_info of a member context
 * (yolo2_hip_multi_ctx) describes its shard */
int  yolo2_hip_multi_loop_images_pix(yolo2_hip_multi *m, int precision, const uint8_t *const *images, const int *widths, const int *heights,
                                     int pixfmt, int n, int batch_per_device, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                     int cap_per_frame, int *counts, int *final_q, const char *const *labels, int n_labels, int out_format,
                                     int quality, uint8_t *const *out, const size_t *caps, size_t *sizes, int *drawn);
/* the same from JPEG streams (see yolo2_hip_loop_images_jpeg) and the records entry from streams (see yolo2_hip_run_images_jpeg_dets):
 * shard i is decoded, run, painted and encoded by device i; the whole call is looked at before a shard starts; frame numbers in the
 * records are global, status [n] is indexed globally, and a shard's error names the frame within the shard beside the shard's first
 * frame; yolo2_hip_jpeg_last_info / _split_info / _loop_last_info of a member context describe its shard.  Option jpegdec_split is
 * each member context's own. */
int  yolo2_hip_multi_loop_images_jpeg(yolo2_hip_multi *m, int precision, const uint8_t *const *streams, const size_t *sizes, int *widths,
                                      int *heights, int n, int batch_per_device, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                      int cap_per_frame, int *counts, int *final_q, const char *const *labels, int n_labels, int out_format,
                                      int quality, uint8_t *const *out, const size_t *caps, size_t *out_sizes, int *drawn, int *status);
int  yolo2_hip_multi_run_images_jpeg_dets(yolo2_hip_multi *m, int precision, const uint8_t *const *streams, const size_t *sizes, int *widths,
                                          int *heights, int n, int batch_per_device, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                          int cap_per_frame, int *counts, int *final_q, int *status);

/* (b) one process per device (torchrun / MPI style; what bench.py --gpus N runs): rank 0 makes the 128-byte id
 * (ncclGetUniqueId), the launcher hands it to every rank, each rank joins with its context (ncclCommInitRank), then
 * ALL ranks call the _bcast loader: the root passes the host blobs and Q tables, the others NULL / 0. */
int  yolo2_hip_rccl_unique_id(void *id128);
int  yolo2_hip_rccl_init_rank(yolo2_hip_ctx *ctx, int device, const void *id128, int nranks, int rank);
void yolo2_hip_rccl_finalize(yolo2_hip_ctx *ctx);
int  yolo2_hip_load_weights_int16_bcast(yolo2_hip_ctx *ctx, const int16_t *weights_reorg, size_t n_weights,
                                        const int16_t *bias, size_t n_bias, const int32_t *weight_q, int n_weight_q,
                                        const int32_t *bias_q, int n_bias_q, const int32_t *act_q, int n_act_q, int root);
int  yolo2_hip_load_weights_fp32_bcast(yolo2_hip_ctx *ctx, const float *weights_reorg, size_t n_weights,
                                       const float *bias, size_t n_bias, int root);
/* Failure of a _bcast loader is COLLECTIVE: every rank first does its local part (the root: argument checks, allocation, H2D;
 * the others: allocation), the ranks agree on a status word (one ncclAllReduce(min) of an int), and either all of them run the
 * broadcast or all of them return an error; a second agreement follows the per-rank load.  A root-side error therefore never
 * leaves the other ranks blocked inside ncclBroadcast.  A rank whose process dies is the launcher's business. */

/* What the communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice / ncclGetVersion), the file the
 * RCCL entry points were resolved from (dladdr: a process that already mapped a librccl with the same soname - torch ships one -
 * gets that copy from dlopen), and the most recent weight broadcast through it.  "Did RCCL see N ranks" is answered by nranks. */
typedef struct {
    int nranks, rank, device;
    int version;                 /* ncclGetVersion: e.g. 22606 */
    int bcasts;                  /* weight broadcasts run through this communicator */
    double last_bcast_ms;        /* host wall time of the last one (enqueue to stream-synchronised), this rank */
    uint64_t last_bcast_bytes;   /* bytes each rank received / the root sent per peer */
    char lib_path[256];
} yolo2_hip_rccl_info_t;
int  yolo2_hip_rccl_info(yolo2_hip_ctx *ctx, yolo2_hip_rccl_info_t *out);
int  yolo2_hip_multi_rccl_info(yolo2_hip_multi *m, yolo2_hip_rccl_info_t *out);   /* model (a): rank/device of member 0 */

/* ------------------------------------------------------------------- tier 3: helpers */

/* The layer table the batched entry implements (config/yolov2.cfg as parsed by
 * src/core/yolo_net.cpp:218-291).  desc = {type, c, h, w, n, size, stride, pad, leaky} with
 * type 0 conv, 1 maxpool, 2 reorg, 3 route, 4 region (linux_app/include/yolo2_config.h:118-122).
 * Hosts that parse a .cfg compare it with this before using yolo2_hip_run_batch_*. */
int yolo2_hip_num_layers(void);
int yolo2_hip_layer_desc(int layer_idx, int desc[9]);
/* ... and how the table is connected: the sources of a [route] layer as absolute layer indices, in the cfg's order.  Returns their
 * number, 0 for a layer that is no route, YOLO2_ERROR for a bad argument.  A cfg whose routes differ describes another network. */
int yolo2_hip_layer_routes(int layer_idx, int src[4]);
/* Test hook: what the library derives from the table and the routes for one layer - {conv ordinal or -1, weight offset, bias offset
 * (elements of the reference streams), layer whose output it reads (-1: the input; routes resolved, the concat tensor is its route
 * layer), route layer of the concat tensor its output lives in or -1, first channel there, number of readers, first reader or -1,
 * 1 if the region layer reads it, C, H, W of the tensor its output lives in}. */
int yolo2_hip_debug_layer_wiring(int layer_idx, int out[12]);

/* weights_reorg_int16.bin / bias_int16.bin carry one pad element after every odd-length
 * layer (yolo2_model.cpp:198-224).  Returns elements written, or -1 if the file is short. */
long yolo2_strip_int16_layer_pad(const int16_t *file, size_t file_elems, const int *layer_len,
                                 int n_layers, int16_t *dst);
extern const int yolo2_weight_len[YOLO2_N_CONV]; /* model_config.cpp:4-7  */
extern const int yolo2_bias_len[YOLO2_N_CONV];   /* model_config.cpp:9-10 */

#ifdef __cplusplus
}
#endif
#endif /* YOLO2_HIP_H */
