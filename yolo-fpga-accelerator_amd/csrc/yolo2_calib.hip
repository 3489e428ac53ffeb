// yolo2_calib.hip -- calibration: from the resident fp32 weights (yolo2_hip_load_weights_fp32) and calibration frames to the
// reference's int16 artefacts - int16 weight / bias streams and the three Q tables (weight_int16_Q, bias_int16_Q, iofm_Q) - which
// go straight into yolo2_hip_load_weights_int16.
//
// Statistics.  The exact fp32 pass (yolo2_fp32.hip) keeps every conv layer's UNPOOLED output in HBM (f_out[i]) and is bit-identical
// to the reference's fp32, so max |x| of its tensors is the reference's own activation range; the fp16 passes never hold layer 0's
// output or the fused 1x1 layers as tensors.  One k_absmax_f32 per tensor after a pass: pad items, lead / tail and the unused lanes
// of a partial channel group are stored zeros and do not move a maximum.  Layer 24 writes into the concat tensor; only its own
// channel-group range is reduced.
//
// Q rule.  q(m, h) = the largest integer q in 0..15 at which h * m still quantises to at most 32767, i.e. h * m * 2^q < 32767.5
// (rounding is half away from zero), evaluated in double; m = 0 gives 15; no such q is an error naming the tensor.  At that q the
// quantiser's clamp changes no value of the tensor.
//     weight_q[ord] = q(max |w_ord|, 1)        bias_q[ord] = q(max |b_ord|, 1)
//     act_q[0]      = q(max |input|, 1)        act_q[ord + 1] = q(max |out_ord|, headroom),  headroom >= 1 (the caller's margin for
//                                              frames the calibration set did not hold)
// Fix-up: the layer loop (yolo2_model.cpp:379-399; resolve_q in yolo2_int16.hip) only ever shifts the reorg half of the concat tensor
// DOWN to layer 24's Q.  If layer 24's output Q came out above layer 26's it is lowered to layer 26's; otherwise the two halves of the
// tensor layer 29 reads would carry different scales.
//
// Quantiser.  int16 = round(x * 2^Q) by the rule of the network input (k_quantize_i16), elementwise on the resident reorganised
// streams: the int16 and fp32 streams have the same element order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "y2_internal.hpp"
#include "kernels_calib.hpp"

using namespace y2;

namespace {

// slot pairs {max bits, non-finite count} of yolo2_hip_ctx::calib_stats
constexpr int kActSlot = 0;                              // 24: the input, then every conv output
constexpr int kWeightSlot = kActSlot + YOLO2_N_CONV + 1; // 23
constexpr int kBiasSlot = kWeightSlot + YOLO2_N_CONV;    // 23
constexpr int kProbeSlot = kBiasSlot + YOLO2_N_CONV;     // the frames of the call in flight, before they may touch the statistics
constexpr int kClampSlot = kProbeSlot + 1;               // [0]: values the quantiser clamped
constexpr int kSlots = kClampSlot + 1;

unsigned calib_grid(long n)
{
    const long b = ((n + 3) / 4 + kCalibBlock - 1) / kCalibBlock;
    return (unsigned)std::min<long>(std::max<long>(b, 1), kCalibMaxGrid);
}

void launch_absmax(const float *x, long n, unsigned *slot, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_absmax_f32, dim3(calib_grid(n)), dim3(kCalibBlock), 0, st, x, n, slot);
}

float bits_float(unsigned u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int ensure_stats(yolo2_hip_ctx *c)
{
    if (c->calib_stats) return YOLO2_SUCCESS;
    const int rc = c->calib_stats.alloc((size_t)kSlots * 2);
    if (rc) return rc;
    HIP_TRY(hipMemset(c->calib_stats.get(), 0, (size_t)kSlots * 2 * sizeof(unsigned)), YOLO2_DMA_ERROR);
    c->calib_frames_seen = 0;
    return YOLO2_SUCCESS;
}

int need_fp32(const yolo2_hip_ctx *c)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    if (!c->f16_loaded || !c->wf32 || !c->bf32) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    return YOLO2_SUCCESS;
}

// the weight and bias maxima of the resident blobs (fresh at every call: a reload never leaves stale values), then all slots to the host
int collect(yolo2_hip_ctx *c, unsigned (&host)[kSlots * 2])
{
    int rc = ensure_stats(c);
    if (rc) return rc;
    unsigned *const s = c->calib_stats.get();
    HIP_TRY(hipMemsetAsync(s + 2 * kWeightSlot, 0, (size_t)2 * YOLO2_N_CONV * 2 * sizeof(unsigned), nullptr), YOLO2_DMA_ERROR);
    for (int o = 0; o < YOLO2_N_CONV; ++o) {
        launch_absmax(c->wf32 + kWire[kConvLayer[o]].w_off, yolo2_weight_len[o], s + 2 * (kWeightSlot + o), nullptr);
        launch_absmax(c->bf32 + kWire[kConvLayer[o]].b_off, yolo2_bias_len[o], s + 2 * (kBiasSlot + o), nullptr);
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpy(host, s, sizeof(host), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

// q(m, h) of the header comment; -1 if no q in 0..15 fits (or m is not a finite non-negative number)
int q_of(double m, double h)
{
    if (!(m >= 0.0) || !std::isfinite(m)) return -1;
    if (m == 0.0) return 15;
    for (int q = 15; q >= 0; --q)
        if (h * m * std::ldexp(1.0, q) < 32767.5) return q;
    return -1;
}

}  // namespace

// One exact fp32 pass over `batch` frames and the 24 reductions, accumulated into the context's statistics; `counted` of the frames
// are new (a padded last chunk repeats its last image, which moves no maximum).  Synchronises `st`.
int y2_calib_frames(yolo2_hip_ctx *c, uint64_t frames_dev, int batch, int counted, hipStream_t st)
{
    int rc = need_fp32(c);
    if (rc) return rc;
    if (!frames_dev) return fail(YOLO2_ERROR, "null buffer address");
    if (frames_dev & 3) return fail(YOLO2_ERROR, "calibration frames start on a 4-byte boundary");
    if (batch <= 0 || batch > 1024) return fail(YOLO2_ERROR, "batch %d out of range", batch);
    if (counted <= 0 || counted > batch) return fail(YOLO2_ERROR, "bad frame count %d of a batch of %d", counted, batch);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if ((rc = ensure_stats(c))) return rc;
    unsigned *const s = c->calib_stats.get();
    // a NaN or Inf in the frames would reach every statistic behind it: look before the pass and refuse with nothing accumulated
    unsigned probe[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(s + 2 * kProbeSlot, 0, 2 * sizeof(unsigned), st), YOLO2_DMA_ERROR);
    launch_absmax((const float *)(uintptr_t)frames_dev, (long)batch * YOLO2_FRAME_ELEMS, s + 2 * kProbeSlot, st);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpyAsync(probe, s + 2 * kProbeSlot, sizeof(probe), hipMemcpyDeviceToHost, st), YOLO2_DMA_ERROR);
    HIP_TRY(hipStreamSynchronize(st), YOLO2_ERROR);
    if (probe[1]) return fail(YOLO2_ERROR, "calibration frames hold %u non-finite values (NaN or Inf); nothing was accumulated", probe[1]);
    Y2DevBuf<float> region;   // the pass wants somewhere to gather its region tensor
    if ((rc = region.alloc((size_t)batch * YOLO2_REGION_ELEMS))) return rc;
    if ((rc = yolo2_hip_run_batch_fp32(c, frames_dev, batch, (uint64_t)(uintptr_t)region.get(), st))) return rc;
    {
        const ActGeom &g = c->f_in.g;
        launch_absmax((const float *)(c->f_in.d + kLead), (long)g.CG * g.cg_stride * 4, s + 2 * kActSlot, st);
    }
    for (int ord = 0; ord < YOLO2_N_CONV; ++ord) {
        const int i = kConvLayer[ord];
        const LayerDesc &l = kNet[i];
        const auto &t = c->f_out[i];
        // the concat's conv member is a view of the concat tensor: its channels start behind the reorg half's
        const long base = y2_conv_io(i, c->f_in, c->f_out).out_base;
        const long items = (long)((l.n + 3) / 4) * t.g.cg_stride;
        if (base + items > t.g.items) return fail(YOLO2_ERROR, "calibration: layer %d's range leaves its tensor", i);
        launch_absmax((const float *)(t.d + base), items * 4, s + 2 * (kActSlot + 1 + ord), st);
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipStreamSynchronize(st), YOLO2_ERROR);   // (also: `region` is freed on return)
    c->calib_frames_seen += counted;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_absmax_f32(uint64_t data_dev, size_t n, float *absmax, uint32_t *nonfinite, void *stream)
{
    if (!data_dev || !absmax) return fail(YOLO2_ERROR, "null argument");
    if (data_dev & 3) return fail(YOLO2_ERROR, "absmax: the float range starts on a 4-byte boundary");
    if (!n || n > ((size_t)1 << 40)) return fail(YOLO2_ERROR, "absmax: bad element count %zu", n);
    hipStream_t st = (hipStream_t)stream;
    Y2DevBuf<unsigned> slot;
    int rc = slot.alloc(2);
    if (rc) return rc;
    unsigned host[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(slot.get(), 0, sizeof(host), st), YOLO2_DMA_ERROR);
    launch_absmax((const float *)(uintptr_t)data_dev, (long)n, slot.get(), st);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpyAsync(host, slot.get(), sizeof(host), hipMemcpyDeviceToHost, st), YOLO2_DMA_ERROR);
    HIP_TRY(hipStreamSynchronize(st), YOLO2_ERROR);
    *absmax = bits_float(host[0]);
    if (nonfinite) *nonfinite = host[1];
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_calib_reset(yolo2_hip_ctx *c)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    c->calib_frames_seen = 0;
    if (!c->calib_stats) return YOLO2_SUCCESS;
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    HIP_TRY(hipMemset(c->calib_stats.get(), 0, (size_t)kSlots * 2 * sizeof(unsigned)), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_calib_frames(yolo2_hip_ctx *c, uint64_t frames_dev, int batch, void *stream)
{
    return y2_calib_frames(c, frames_dev, batch, batch, (hipStream_t)stream);
}

extern "C" int yolo2_hip_calib_stats(yolo2_hip_ctx *c, float *act_absmax, float *weight_absmax, float *bias_absmax, long *frames_seen)
{
    int rc = need_fp32(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    unsigned h[kSlots * 2];
    if ((rc = collect(c, h))) return rc;
    for (int i = 0; i <= YOLO2_N_CONV && act_absmax; ++i) act_absmax[i] = bits_float(h[2 * (kActSlot + i)]);
    for (int i = 0; i < YOLO2_N_CONV && weight_absmax; ++i) weight_absmax[i] = bits_float(h[2 * (kWeightSlot + i)]);
    for (int i = 0; i < YOLO2_N_CONV && bias_absmax; ++i) bias_absmax[i] = bits_float(h[2 * (kBiasSlot + i)]);
    if (frames_seen) *frames_seen = c->calib_frames_seen;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_calib_q_from_stats(const float *act_absmax, const float *weight_absmax, const float *bias_absmax, float headroom,
                                            int32_t *weight_q, int32_t *bias_q, int32_t *act_q)
{
    if (!act_absmax || !weight_absmax || !bias_absmax || !weight_q || !bias_q || !act_q) return fail(YOLO2_ERROR, "null argument");
    if (!(headroom >= 1.0f) || !std::isfinite(headroom)) return fail(YOLO2_ERROR, "headroom %g is not a finite number >= 1", (double)headroom);
    for (int o = 0; o < YOLO2_N_CONV; ++o) {
        if ((weight_q[o] = q_of(weight_absmax[o], 1.0)) < 0)
            return fail(YOLO2_ERROR, "no Q in 0..15 holds the weights of conv %d (max |w| = %g)", o, (double)weight_absmax[o]);
        if ((bias_q[o] = q_of(bias_absmax[o], 1.0)) < 0)
            return fail(YOLO2_ERROR, "no Q in 0..15 holds the biases of conv %d (max |b| = %g)", o, (double)bias_absmax[o]);
    }
    if ((act_q[0] = q_of(act_absmax[0], 1.0)) < 0) return fail(YOLO2_ERROR, "no Q in 0..15 holds the network input (max = %g)", (double)act_absmax[0]);
    for (int ord = 0; ord < YOLO2_N_CONV; ++ord)
        if ((act_q[ord + 1] = q_of(act_absmax[ord + 1], headroom)) < 0)
            return fail(YOLO2_ERROR, "no Q in 0..15 holds the output of conv %d (layer %d, max = %g, headroom %g)", ord, kConvLayer[ord],
                        (double)act_absmax[ord + 1], (double)headroom);
    // the concat fix-up (header comment): the reorg half is only ever shifted down to the Q of the concat's conv member
    const int q_conv = kWire[kWiring.cat_conv].ord + 1, q_feed = kWire[kWiring.cat_feed].ord + 1;
    if (act_q[q_conv] > act_q[q_feed]) act_q[q_conv] = act_q[q_feed];
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_calib_q_tables(yolo2_hip_ctx *c, float headroom, int32_t *weight_q, int32_t *bias_q, int32_t *act_q)
{
    int rc = need_fp32(c);
    if (rc) return rc;
    if (!weight_q || !bias_q || !act_q) return fail(YOLO2_ERROR, "null argument");
    if (!(headroom >= 1.0f) || !std::isfinite(headroom)) return fail(YOLO2_ERROR, "headroom %g is not a finite number >= 1", (double)headroom);
    if (c->calib_frames_seen <= 0) return fail(YOLO2_ERROR, "no calibration frame seen (yolo2_hip_calib_frames)");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    unsigned h[kSlots * 2];
    if ((rc = collect(c, h))) return rc;
    float act[YOLO2_N_CONV + 1], w[YOLO2_N_CONV], b[YOLO2_N_CONV];
    for (int i = 0; i <= YOLO2_N_CONV; ++i) {
        if (h[2 * (kActSlot + i) + 1])
            return fail(YOLO2_ERROR, "%u non-finite values in activation tensor %d (0 = the input, k = the output of conv k-1)",
                        h[2 * (kActSlot + i) + 1], i);
        act[i] = bits_float(h[2 * (kActSlot + i)]);
    }
    for (int i = 0; i < YOLO2_N_CONV; ++i) {
        if (h[2 * (kWeightSlot + i) + 1]) return fail(YOLO2_ERROR, "%u non-finite weights in conv %d", h[2 * (kWeightSlot + i) + 1], i);
        if (h[2 * (kBiasSlot + i) + 1]) return fail(YOLO2_ERROR, "%u non-finite biases in conv %d", h[2 * (kBiasSlot + i) + 1], i);
        w[i] = bits_float(h[2 * (kWeightSlot + i)]);
        b[i] = bits_float(h[2 * (kBiasSlot + i)]);
    }
    return yolo2_hip_calib_q_from_stats(act, w, b, headroom, weight_q, bias_q, act_q);
}

// ---- the int8 pass's Q rule (include/yolo2_hip.h "int8 pass"): the rule above with the int8 limit and a range of -8..24

// q8(m, h); INT_MIN-like -100 if no q in -8..24 fits (or m is not a finite non-negative number)
static int q8_of(double m, double h)
{
    if (!(m >= 0.0) || !std::isfinite(m)) return -100;
    if (m == 0.0) return 24;
    for (int q = 24; q >= -8; --q)
        if (h * m * std::ldexp(1.0, q) < 127.5) return q;
    return -100;
}

extern "C" int yolo2_hip_calib_q8_from_stats(const float *act_absmax, float headroom, int32_t *act_q)
{
    if (!act_absmax || !act_q) return fail(YOLO2_ERROR, "null argument");
    if (!(headroom >= 1.0f) || !std::isfinite(headroom)) return fail(YOLO2_ERROR, "headroom %g is not a finite number >= 1", (double)headroom);
    if ((act_q[0] = q8_of(act_absmax[0], 1.0)) == -100)
        return fail(YOLO2_ERROR, "no Q in -8..24 holds the network input (max = %g)", (double)act_absmax[0]);
    for (int o = 0; o < YOLO2_N_CONV; ++o)
        if ((act_q[o + 1] = q8_of(act_absmax[o + 1], headroom)) == -100)
            return fail(YOLO2_ERROR, "no Q in -8..24 holds the output of conv %d (max = %g, headroom %g)", o, (double)act_absmax[o + 1],
                        (double)headroom);
    // both halves of the concat tensor (its conv member, and the conv its reorg member reads) take the smaller Q: nothing is shifted at run time
    const int q_conv = kWire[kWiring.cat_conv].ord + 1, q_feed = kWire[kWiring.cat_feed].ord + 1;
    act_q[q_conv] = act_q[q_feed] = std::min(act_q[q_conv], act_q[q_feed]);
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_calib_q8_tables(yolo2_hip_ctx *c, float headroom, int32_t *act_q)
{
    int rc = need_fp32(c);
    if (rc) return rc;
    if (!act_q) return fail(YOLO2_ERROR, "null argument");
    if (!(headroom >= 1.0f) || !std::isfinite(headroom)) return fail(YOLO2_ERROR, "headroom %g is not a finite number >= 1", (double)headroom);
    if (c->calib_frames_seen <= 0) return fail(YOLO2_ERROR, "no calibration frame seen (yolo2_hip_calib_frames)");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    unsigned h[kSlots * 2];
    if ((rc = collect(c, h))) return rc;
    float act[YOLO2_N_CONV + 1];
    for (int i = 0; i <= YOLO2_N_CONV; ++i) {
        if (h[2 * (kActSlot + i) + 1])
            return fail(YOLO2_ERROR, "%u non-finite values in activation tensor %d (0 = the input, k = the output of conv k-1)",
                        h[2 * (kActSlot + i) + 1], i);
        act[i] = bits_float(h[2 * (kActSlot + i)]);
    }
    return yolo2_hip_calib_q8_from_stats(act, headroom, act_q);
}

extern "C" int yolo2_hip_quantize_weights_int16(yolo2_hip_ctx *c, const int32_t *weight_q, const int32_t *bias_q, int16_t *weights_reorg_out,
                                                size_t n_weights, int16_t *bias_out, size_t n_bias, long *clamped)
{
    int rc = need_fp32(c);
    if (rc) return rc;
    if (!weight_q || !bias_q || !weights_reorg_out || !bias_out) return fail(YOLO2_ERROR, "null argument");
    if (n_weights < (size_t)YOLO2_N_WEIGHTS || n_bias < (size_t)YOLO2_N_BIAS)
        return fail(YOLO2_ERROR, "output buffers of %zu / %zu elements are short of %d weights / %d biases", n_weights, n_bias, YOLO2_N_WEIGHTS,
                    YOLO2_N_BIAS);
    for (int o = 0; o < YOLO2_N_CONV; ++o)
        if (weight_q[o] < 0 || weight_q[o] > 30 || bias_q[o] < 0 || bias_q[o] > 30)
            return fail(YOLO2_ERROR, "Q of conv %d out of range 0..30 (weights %d, biases %d)", o, weight_q[o], bias_q[o]);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if ((rc = ensure_stats(c))) return rc;
    unsigned *const slot = c->calib_stats.get() + 2 * kClampSlot;
    Y2DevBuf<short> wq, bq;
    if ((rc = wq.alloc(YOLO2_N_WEIGHTS)) || (rc = bq.alloc(YOLO2_N_BIAS))) return rc;
    HIP_TRY(hipMemsetAsync(slot, 0, 2 * sizeof(unsigned), nullptr), YOLO2_DMA_ERROR);
    for (int o = 0; o < YOLO2_N_CONV; ++o) {
        const long nw = yolo2_weight_len[o], nb = yolo2_bias_len[o], woff = kWire[kConvLayer[o]].w_off, boff = kWire[kConvLayer[o]].b_off;
        hipLaunchKernelGGL(k_quantize_i16, dim3(calib_grid(nw)), dim3(kCalibBlock), 0, nullptr, (const float *)(c->wf32 + woff), wq.get() + woff,
                           nw, (int)weight_q[o], slot);
        hipLaunchKernelGGL(k_quantize_i16, dim3(calib_grid(nb)), dim3(kCalibBlock), 0, nullptr, (const float *)(c->bf32 + boff), bq.get() + boff,
                           nb, (int)bias_q[o], slot);
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    unsigned n_clamped = 0;
    HIP_TRY(hipMemcpy(weights_reorg_out, wq.get(), (size_t)YOLO2_N_WEIGHTS * sizeof(int16_t), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(bias_out, bq.get(), (size_t)YOLO2_N_BIAS * sizeof(int16_t), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(&n_clamped, slot, sizeof(n_clamped), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    if (clamped) *clamped = (long)n_clamped;
    return YOLO2_SUCCESS;
}
