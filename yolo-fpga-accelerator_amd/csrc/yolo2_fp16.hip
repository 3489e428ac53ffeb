// yolo2_fp16.hip -- the fp16 MFMA path of libyolo2_hip.so (config C4): the floating-point form of the same network as
// implicit-GEMM convolutions on the matrix cores (csrc/kernels_f16.hpp).  Weight packing (also keeps the fp32 blobs resident
// for yolo2_fp32.hip), the per-context launch table and yolo2_hip_run_batch_fp16.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "y2_internal.hpp"
#include "kernels_f16.hpp"

using namespace y2;

// ---------------------------------------------------------------------------- the launch table
//
// Which kernel runs which layer is decided ONCE per (context, batch) and stored as a table of steps; a pass is a walk over
// that table (no environment look-ups, no selection logic on the launch path).  The A/B switches of the kernel families
// (options f16_* of the context, from YOLO2_F16_* at context creation or yolo2_hip_set_option: tests and tools/abenv.sh use
// them) are latched once, when the weights are loaded, into F16Switches.

struct F16Switches {
    int lanes = 2;            // YOLO2_F16_LANES=n (1..8), YOLO2_F16_NO_LANES -> 1
    bool no_mfma0 = false, no_glds = false, no_poolfuse = false, no_halo = false, no_persist = false, persist_all = false;
    bool ring_all = false, no_ring = false, no_c32 = false, m16 = false, w8 = false, no_wide = false;
    int stamp_layer = -1;     // diagnostic builds (-DY2_STAMPS): the layer whose halo launch records its workgroup timeline
    bool verbose = false;
    int skip = 0;             // diagnostic: see Y2Options::f16_skip
    bool no_fuse1x1 = false, no_rw = false, no_rwb = false, no_rwc = false, ring256 = false, ring_sq = false;
    static F16Switches from_options(const Y2Options &o)   // the context's option set (y2_internal.hpp), latched at weight load
    {
        F16Switches s;
        s.lanes = o.f16_no_lanes ? 1 : o.f16_lanes;
        s.no_mfma0 = o.f16_no_mfma0; s.no_glds = o.f16_no_glds; s.no_poolfuse = o.f16_no_poolfuse;
        s.no_halo = o.f16_no_halo; s.no_persist = o.f16_no_persist; s.persist_all = o.f16_persist_all;
        s.ring_all = o.f16_ring_all; s.no_ring = o.f16_no_ring; s.no_c32 = o.f16_no_c32;
        s.m16 = o.f16_m16; s.w8 = o.f16_w8; s.no_wide = o.f16_no_wide;
        s.no_fuse1x1 = o.f16_no_fuse1x1; s.no_rw = o.f16_no_rw; s.no_rwb = o.f16_no_rwb; s.no_rwc = o.f16_no_rwc; s.ring256 = o.f16_ring256; s.ring_sq = o.f16_ring_sq;
        s.stamp_layer = o.stamp_layer;
        s.verbose = o.verbose;
        s.skip = o.f16_skip;
        return s;
    }
};

struct F16Step;
typedef void (*F16Launch)(const F16Step &, const float *frames, float *region, hipStream_t);

// How a kernel family stores its output (what the extent check below needs to know about it)
enum F16Store {
    FS_FULL = 0,       // full-resolution items at the conv's own geometry (a.PL / a.Wp); IGNORES a.pool
    FS_FULL_OR_POOL,   // honours a.pool: pooled items at (a.oPL / a.oWp) when set, full-resolution otherwise
    FS_POOL_ONLY,      // always stores the pooled tensor (fused conv + pool kernels)
    FS_REGION,         // dense fp32 [B][N][H][W] into the caller's region buffer (extent = the caller's contract)
};

struct F16Step {
    int layer = 0;               // network layer whose hipEvent slot this launch is booked to
    const char *kernel = "";
    F16Launch launch = nullptr;
    F16Store store = FS_FULL;
    ConvF16Args a;
    dim3 grid, block;
    unsigned lds = 0;
    int lt_rows = 0, T = 0;      // extra kernel arguments (halo tile rows, persistent kernels' tile count)
    const _Float16 *in = nullptr, *w = nullptr, *w2 = nullptr;     // w2 / bias2: the 1x1 layer fused behind a 3x3 (k_conv_f16_rw MODE 2)
    const float *bias = nullptr, *w0 = nullptr, *bias2 = nullptr;
    _Float16 *out = nullptr;
    int B = 0;
    // pool / reorg steps: source and destination geometry (iPS / oPS: part strides of split items)
    int iCp = 0, iWp = 0, iPL = 0, oCp = 0, oWp = 0, oPL = 0, OH = 0, OW = 0, iPS = 0, oPS = 0;
};

typedef void (*F16LaunchU8)(const F16Step &, const uint8_t *lb, int lb_first, hipStream_t);

struct F16Plan {
    F16Switches sw;
    int batch = 0;               // the batch the table below was built for (0 = none)
    std::vector<F16Step> steps;
    // the images entries' layer-0 step "from bytes" (layers 0+1 from a chunk's staging buffer), used instead of steps[0]; every
    // other step is the table's.  Not set (launch_u8 == nullptr) under f16_no_mfma0: those entries letterbox into frames first.
    // launch_yuyv / yuyv_kernel: the same step "from YUYV bytes" (a chunk of packed YUYV 4:2:2 frames: k_conv0_pool_mfma_yuyv).
    F16Step u8;
    F16LaunchU8 launch_u8 = nullptr, launch_yuyv = nullptr;
    const char *yuyv_kernel = "";
};

void y2_f16_plan_free(yolo2_hip_ctx *c)
{
    delete c->f16_plan;
    c->f16_plan = nullptr;
}

// The launch-time extent check.  Every step that stores into one of the context's tensors must (a) address it with that
// tensor's own pitches, (b) cover no more pixels than it holds and (c) stay inside its item.  In round 2 a kernel that ignores
// ConvF16Args::pool (the persistent halo kernel) was, for one commit, routed to layer 6 while the layer's pooled tensor was
// passed as its output: full-resolution offsets (104 x 104 planes) into a 52 x 52 tensor = an out-of-bounds store, a GPU memory
// fault and an abort inside run_batch_fp16.  This check turns that class of mistake into YOLO2_ERROR before
// anything is launched; yolo2_hip_f16_store_check exposes it so that it can be tested without a GPU.
#ifndef Y2_CONV0_WGS
#define Y2_CONV0_WGS 4
#endif

static int f16_store_check(const char *kernel, int store, int pool, int B, int H, int W, int Cp_out, int out_ch_off, int n_store,
                           int oWp, int oPL, int npix, int npool, int dst_B, int dst_H, int dst_W, int dst_Cp, int split_n = 0)
{
    if (store == FS_REGION) return YOLO2_SUCCESS;
    const bool pooled = store == FS_POOL_ONLY || (store == FS_FULL_OR_POOL && pool);
    if (store == FS_FULL && pool)
        return fail(YOLO2_ERROR, "fp16 plan: %s stores the full-resolution tensor and cannot fuse the pool (ConvF16Args::pool is set)", kernel);
    const int sH = pooled ? H / 2 : H, sW = pooled ? W / 2 : W;           // geometry the kernel's stores follow
    const int sWp = pooled ? oWp : W + 1, sPL = pooled ? oPL : (H + 1) * (W + 1), sN = pooled ? npool : npix;
    if (dst_B != B || dst_H != sH || dst_W != sW)
        return fail(YOLO2_ERROR, "fp16 plan: %s would store %d x %d x %d pixels into a tensor of %d x %d x %d", kernel, B, sH, sW, dst_B, dst_H, dst_W);
    if (sWp != dst_W + 1 || sPL != (dst_H + 1) * (dst_W + 1) || sN != dst_B * dst_H * dst_W)
        return fail(YOLO2_ERROR, "fp16 plan: %s addresses its output with pitch %d / plane %d / %d pixels, the tensor has %d / %d / %d", kernel,
                    sWp, sPL, sN, dst_W + 1, (dst_H + 1) * (dst_W + 1), dst_B * dst_H * dst_W);
    if (Cp_out != dst_Cp || out_ch_off < 0 || n_store < 0 || out_ch_off + n_store > dst_Cp)
        return fail(YOLO2_ERROR, "fp16 plan: %s stores channels [%d, %d) of %d-channel items into %d-channel items", kernel, out_ch_off,
                    out_ch_off + n_store, Cp_out, dst_Cp);
    // split mode: the same channel window in each of the three parts [hi | lo | hi] of split_n channels
    if (split_n && (split_n < out_ch_off + n_store || 2 * split_n + out_ch_off + n_store > dst_Cp))
        return fail(YOLO2_ERROR, "fp16 plan (split): %s stores channels [%d, %d) of three parts of %d channels into %d-channel items", kernel,
                    out_ch_off, out_ch_off + n_store, split_n, dst_Cp);
    return YOLO2_SUCCESS;
}

// Test hook (no GPU needed): the check above on explicit numbers.  store: 0 full-resolution only, 1 full or pooled
// (honours `pool`), 2 pooled only.  Returns YOLO2_SUCCESS or YOLO2_ERROR with yolo2_hip_last_error() set.
extern "C" int yolo2_hip_f16_store_check(int store, int pool, int B, int H, int W, int Cp_out, int out_ch_off, int n_store, int dst_B,
                                         int dst_H, int dst_W, int dst_Cp)
{
    if (store < 0 || store > 2) return fail(YOLO2_ERROR, "bad store kind %d", store);
    return f16_store_check("kernel", store, pool, B, H, W, Cp_out, out_ch_off, n_store, W / 2 + 1, (H / 2 + 1) * (W / 2 + 1), B * H * W,
                           B * (H / 2) * (W / 2), dst_B, dst_H, dst_W, dst_Cp);
}


static int load_fp32_common(yolo2_hip_ctx *c, const void *weights_reorg, size_t n_weights, const void *bias, size_t n_bias, hipMemcpyKind kind);

extern "C" int yolo2_hip_load_weights_fp32(yolo2_hip_ctx *c, const float *weights_reorg, size_t n_weights,
                                           const float *bias, size_t n_bias)
{
    return load_fp32_common(c, weights_reorg, n_weights, bias, n_bias, hipMemcpyHostToDevice);
}

extern "C" int yolo2_hip_load_weights_fp32_dev(yolo2_hip_ctx *c, uint64_t weights_reorg_dev, size_t n_weights, uint64_t bias_dev,
                                               size_t n_bias)
{
    return load_fp32_common(c, (const void *)(uintptr_t)weights_reorg_dev, n_weights, (const void *)(uintptr_t)bias_dev, n_bias,
                            hipMemcpyDeviceToDevice);
}

// Item size (halves) of a tensor of C channels: plain fp16 items are C rounded up to 32; split items ("fp32tol" mode) are three parts
// [hi | lo | hi] of PS = C rounded up to 32 channels each, the whole rounded up to the 64-channel K-step of the LDS-DMA kernels.
static inline int part_stride(int C) { return round_up(C, 32); }
static inline int item_halves(int C, bool split) { return split ? round_up(3 * part_stride(C), 64) : part_stride(C); }

// Packs the fp32 blobs (device, reference stream order) into this context's fp16 weight layout: [N_pad][tap][Cp] halves, plain or
// split ([w_hi | w_hi | w_lo] against activations [a_hi | a_lo | a_hi]).  Replaces c->wh / c->biasf and resets the launch table.
static int pack_half_weights(yolo2_hip_ctx *c, const float *wd, const float *bd)
{
    long wtot = 0, btot = 0;
    int ord = 0;
    for (int i = 0; i < 32; ++i)
        if (kNet[i].type == L_CONV) {
            const LayerDesc &l = kNet[i];
            const int npad = round_up(l.n, l.n <= 64 ? 64 : kBN);
            c->wh_off[ord] = wtot;
            c->biasf_off[ord] = btot;
            wtot += i == 0 ? (long)npad * 32 : (long)npad * l.size * l.size * item_halves(l.c, c->split);
            btot += npad;
            ord++;
        }
    for (yolo2_hip_ctx *l : c->f16_lanes) yolo2_hip_destroy(l);   // they alias the buffers that are about to be replaced
    c->f16_lanes.clear();
    y2_f16_plan_free(c);
    c->f16_plan = new (std::nothrow) F16Plan();
    if (!c->f16_plan) return fail(YOLO2_ERROR, "out of host memory");
    c->f16_plan->sw = F16Switches::from_options(c->opt);   // the ONLY place the fp16 path reads its switches
    int rc;
    c->wh_own.reset();
    c->biasf_own.reset();
    c->wh = nullptr;
    c->biasf = nullptr;
    if ((rc = y2_alloc_owned(c->wh_own, c->wh, (size_t)wtot)) || (rc = y2_alloc_owned(c->biasf_own, c->biasf, (size_t)btot))) return rc;
    long woff = 0, boff = 0;
    ord = 0;
    for (int i = 0; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        if (l.type != L_CONV) continue;
        const int npad = round_up(l.n, l.n <= 64 ? 64 : kBN), KK = l.size * l.size;
        if (c->split && i > 0) {
            const int Cp = item_halves(l.c, true);
            const long n = (long)npad * KK * Cp;
            hipLaunchKernelGGL(k_pack_weights_split, dim3(blocks_for(std::max<long>(n, npad), 256)), dim3(256), 0, nullptr, wd + woff,
                               c->wh + c->wh_off[ord], c->biasf + c->biasf_off[ord], bd + boff, l.c, l.n, KK, part_stride(l.c), Cp, npad);
        } else {
            const int Cp = i == 0 ? 32 : round_up(l.c, 32);
            const long n = (long)npad * (i == 0 ? 1 : KK) * Cp;
            hipLaunchKernelGGL(k_pack_weights_f16, dim3(blocks_for(std::max<long>(n, npad), 256)), dim3(256), 0, nullptr, wd + woff,
                               c->wh + c->wh_off[ord], c->biasf + c->biasf_off[ord], bd + boff, l.c, l.n, KK, Cp, npad, i == 0 ? 1 : 0);
        }
        woff += yolo2_weight_len[ord];
        boff += yolo2_bias_len[ord];
        ord++;
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

static int load_fp32_common(yolo2_hip_ctx *c, const void *weights_reorg, size_t n_weights, const void *bias, size_t n_bias, hipMemcpyKind kind)
{
    if (!c || !weights_reorg || !bias) return fail(YOLO2_ERROR, "null argument");
    if (n_weights < YOLO2_N_WEIGHTS) return fail(YOLO2_ERROR, "weights file too small");
    if (n_bias < YOLO2_N_BIAS) return fail(YOLO2_ERROR, "bias file too small");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if (c->tol) { yolo2_hip_destroy(c->tol); c->tol = nullptr; }   // the split-mode twin packs from the blobs that are about to be replaced
    Y2DevBuf<float> wd_own, bd_own;
    int rc;
    if ((rc = wd_own.alloc(YOLO2_N_WEIGHTS)) || (rc = bd_own.alloc(YOLO2_N_BIAS))) return rc;
    float *const wd = wd_own.get(), *const bd = bd_own.get();
    HIP_TRY(hipMemcpy(wd, weights_reorg, (size_t)YOLO2_N_WEIGHTS * 4, kind), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(bd, bias, (size_t)YOLO2_N_BIAS * 4, kind), YOLO2_DMA_ERROR);
    if ((rc = pack_half_weights(c, wd, bd))) return rc;
    // the halo-tile kernels use up to the whole 160 KiB of LDS: raise their dynamic-LDS limit on THIS device
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<128, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<256, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<256, 2, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<256, 2, 16, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo_p<256, 16, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo_p<256, 16, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo_p<128, 8, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo_p<128, 8, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<128, 3, 8, 32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<256, 2, 16, 32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo_p<256, 16, 32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo_p<128, 8, 32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_halo<256, 2, 16, 32, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_rw<13, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_rw<13, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_rw<13, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_rwb<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_rwb<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_conv_f16_rwc, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_gemm1_f16_p<256, 64, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_gemm1_f16_p<256, 128, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_gemm1_f16_p<128, 256, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    HIP_TRY(hipFuncSetAttribute((const void *)k_gemm1_f16_p<256, 256, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    if (!c->w0f && (rc = y2_alloc_owned(c->w0f_own, c->w0f, 27 * 32 + 32))) return rc;
    hipLaunchKernelGGL(k_pack_w0_f32, dim3(4), dim3(256), 0, nullptr, wd, bd, c->w0f, c->w0f + 27 * 32);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    // the fp32 blobs stay resident (204 MB of 288 GB): yolo2_hip_run_frame_fp32_host consumes them as they are
    c->wpkf_own.reset();         // the tiled fp32 path re-packs from the new blobs at its next run
    c->biasf32_pk_own.reset();
    c->wpkf = c->biasf32_pk = nullptr;
    c->wf32_own = std::move(wd_own);
    c->bf32_own = std::move(bd_own);
    c->wf32 = wd;
    c->bf32 = bd;
    c->f16_loaded = true;
    return YOLO2_SUCCESS;
}

static int alloc_half(yolo2_hip_ctx::HalfTensor &t, int C, int Cp, int H, int W, int B)
{
    t.C = C; t.Cp = Cp; t.H = H; t.W = W; t.Wp = W + 1; t.PL = (H + 1) * t.Wp; t.B = B;
    t.items = (size_t)kLead + (size_t)B * t.PL + kTail;
    const int rc = y2_alloc_owned(t.own, t.d, t.items * Cp);
    if (rc) return rc;
    HIP_TRY(hipMemset(t.d, 0, t.items * Cp * 2), YOLO2_DMA_ERROR);  // zeros = conv padding and channel padding
    return YOLO2_SUCCESS;
}

static int ensure_f16_batch(yolo2_hip_ctx *c, int B)
{
    if (c->f16_batch == B) return YOLO2_SUCCESS;
    y2_free_tensors(c->h_in, c->h_out, c->h_cat, c->f16_batch);
    if (c->f16_plan) { c->f16_plan->batch = 0; c->f16_plan->steps.clear(); }   // the table points into the tensors just freed
    int rc;
    if ((rc = alloc_half(c->h_cat, 1280, item_halves(1280, c->split), 13, 13, B))) return rc;
    for (int i = 1; i < 30; ++i) {   // layer 0's 416x416x32 tensor never exists: conv0+pool are fused
        const LayerDesc &l = kNet[i];
        if (l.type == L_CONV && i != 24) {
            if ((rc = alloc_half(c->h_out[i], l.n, item_halves(l.n, c->split), l.h, l.w, B))) return rc;
        } else if (l.type == L_MAX) {
            if ((rc = alloc_half(c->h_out[i], l.c, item_halves(l.c, c->split), l.h / 2, l.w / 2, B))) return rc;
        }
    }
    y2_view_of(c->h_out[24], c->h_cat);
    y2_view_of(c->h_out[27], c->h_cat);
    c->f16_batch = B;
    // the zero fills above run on the null stream; the pass may be enqueued on a non-blocking stream (the lanes'
    // are), which does not order itself behind it
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// ---- launchers: one per kernel instantiation, all with the table's signature
#define Y2_LAUNCHER(name, ...)                                                                         \
    static void name(const F16Step &s, const float *frames, float *region, hipStream_t st)           \
    {                                                                                                  \
        (void)frames; (void)region;                                                                    \
        __VA_ARGS__;                                                                                   \
    }
template <bool SP = false> Y2_LAUNCHER(L_conv0_mfma, hipLaunchKernelGGL(k_conv0_pool_mfma<SP>, s.grid, s.block, 0, st, frames, s.w0, s.bias, s.out, 416, 416, s.oWp, s.oPL, s.T))
template <bool SP>
static void L_conv0_mfma_u8(const F16Step &s, const uint8_t *lb, int lb_first, hipStream_t st)
{
    hipLaunchKernelGGL(k_conv0_pool_mfma_u8<SP>, s.grid, s.block, 0, st, lb, lb_first, s.w0, s.bias, s.out, s.oWp, s.oPL, s.T);
}
template <bool SP>
static void L_conv0_mfma_yuyv(const F16Step &s, const uint8_t *lb, int lb_first, hipStream_t st)
{
    hipLaunchKernelGGL(k_conv0_pool_mfma_yuyv<SP>, s.grid, s.block, 0, st, lb, lb_first, s.w0, s.bias, s.out, s.oWp, s.oPL, s.T);
}
template <bool SP> Y2_LAUNCHER(L_conv0_valu, hipLaunchKernelGGL(k_conv0_pool_f16<SP>, s.grid, s.block, 0, st, frames, s.w0, s.bias, s.out, s.B, 416, 416, s.oWp, s.oPL))
template <int BN> Y2_LAUNCHER(L_ring, hipLaunchKernelGGL((k_gemm1_f16_p<256, BN, 3>), s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out,
                                                            s.store == FS_REGION ? region : (float *)nullptr, s.a, s.T))
Y2_LAUNCHER(L_ring_sq, hipLaunchKernelGGL((k_gemm1_f16_p<256, 256, 2>), s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, (float *)nullptr, s.a, s.T))
Y2_LAUNCHER(L_ring256, hipLaunchKernelGGL((k_gemm1_f16_p<128, 256, 3>), s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, (float *)nullptr, s.a, s.T))
Y2_LAUNCHER(L_c32_pool, hipLaunchKernelGGL(k_conv_f16_c32_pool, s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, s.a, s.T))
Y2_LAUNCHER(L_rwc, hipLaunchKernelGGL(k_conv_f16_rwc, s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, s.a, s.lt_rows, s.T))
template <int BN, bool SP = false> Y2_LAUNCHER(L_glds, hipLaunchKernelGGL((k_conv_f16_glds<BN, SP>), s.grid, s.block, 0, st, s.in, s.w, s.bias, s.out,
                                                                            s.store == FS_REGION ? region : (float *)nullptr, s.a))
template <int BN, int BK> Y2_LAUNCHER(L_reg, hipLaunchKernelGGL((k_conv_f16<128, BN, BK>), s.grid, s.block, 0, st, s.in, s.w, s.bias, s.out,
                                                                   s.store == FS_REGION ? region : (float *)nullptr, s.a))
template <int BN, int NW, int TS, bool SP = false> Y2_LAUNCHER(L_halo_p, hipLaunchKernelGGL((k_conv_f16_halo_p<BN, NW, TS, SP>), s.grid, s.block, s.lds, st, s.in, s.w,
                                                                                            s.bias, s.out, s.a, s.lt_rows, s.T))
template <int BN, int NB, int NW, int TS, bool SP = false, bool F1 = false>
Y2_LAUNCHER(L_halo, hipLaunchKernelGGL((k_conv_f16_halo<BN, NB, NW, TS, SP, F1>), s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, s.a, s.lt_rows, s.w2, s.bias2))
template <int MODE> Y2_LAUNCHER(L_rw, hipLaunchKernelGGL((k_conv_f16_rw<13, MODE>), s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, s.w2, s.bias2, s.a,
                                                       s.lt_rows, s.T))
template <int MODE> Y2_LAUNCHER(L_rwb, hipLaunchKernelGGL((k_conv_f16_rwb<MODE>), s.grid, s.block, s.lds, st, s.in, s.w, s.bias, s.out, s.w2, s.bias2, s.a, s.T))
Y2_LAUNCHER(L_maxpool_split, hipLaunchKernelGGL(k_maxpool2_split, s.grid, s.block, 0, st, s.in, s.out, s.oPS, s.oCp, s.B, s.OH, s.OW, s.iWp, s.iPL, s.oWp, s.oPL))
Y2_LAUNCHER(L_reorg_split, hipLaunchKernelGGL(k_reorg_split, s.grid, s.block, 0, st, s.in, s.out, s.B, s.iPS, s.iCp, s.iWp, s.iPL, s.oPS, s.oCp, s.oWp, s.oPL))
Y2_LAUNCHER(L_maxpool, hipLaunchKernelGGL(k_maxpool2_f16, s.grid, s.block, 0, st, s.in, s.out, s.oCp, s.B, s.OH, s.OW, s.iWp, s.iPL, s.oWp, s.oPL))
Y2_LAUNCHER(L_reorg, hipLaunchKernelGGL(k_reorg_f16, s.grid, s.block, 0, st, s.in, s.out, s.B, s.iCp, s.iWp, s.iPL, s.oCp, s.oWp, s.oPL))
#undef Y2_LAUNCHER

// Builds the table for batch B (the tensors exist: ensure_f16_batch).  The selection rules are those measured in rounds 1-2
// (DESIGN.md 4.3); every conv step passes f16_store_check against the tensor it is handed before it enters the table.
static int build_f16_plan(yolo2_hip_ctx *c, int B)
{
    F16Plan &P = *c->f16_plan;
    const F16Switches &sw = P.sw;
    P.steps.clear();
    P.batch = 0;
    P.launch_u8 = P.launch_yuyv = nullptr;
    typedef yolo2_hip_ctx::HalfTensor HT;
    const bool split = c->split;     // "fp32tol" mode: items of three parts [hi | lo | hi], SPLIT kernel instantiations
    auto checked_push = [&](F16Step &s, const HT &dst) -> int {
        const int rc = f16_store_check(s.kernel, s.store, s.a.pool, B, s.a.H, s.a.W, s.a.Cp_out, s.a.out_ch_off, s.a.n_store, s.a.oWp, s.a.oPL,
                                       s.a.npix, s.a.npool, dst.B, dst.H, dst.W, dst.Cp, s.store == FS_REGION ? 0 : s.a.split_n);
        if (rc) return rc;
        P.steps.push_back(s);
        return YOLO2_SUCCESS;
    };
    {   // layers 0+1 fused: conv 3->32 + leaky + 2x2 pool straight from the float frames
        const HT &g = c->h_out[1];
        F16Step s;
        s.layer = 0; s.B = B;   // (booked to layer 0; the pool, layer 1, has no launch of its own)
        s.w0 = c->w0f; s.bias = c->w0f + 27 * 32; s.out = g.d; s.oWp = g.Wp; s.oPL = g.PL;
        s.block = dim3(256);
        if (split && !sw.no_mfma0) {   // the MFMA form on (hi, lo) pairs: three MFMAs per product, (hi, lo) out: 128-halve items
            s.kernel = "k_conv0_pool_mfma<split>"; s.launch = L_conv0_mfma<true>;
            s.T = B * (416 / 16) * (416 / 32);
            s.grid = dim3((unsigned)std::min(s.T, 256 * 3));   // 161 registers: three workgroups per CU are resident - a fourth would run behind them
        } else if (split) {   // fp32 VALU form, nothing rounded before the pool (option f16_no_mfma0)
            s.kernel = "k_conv0_pool_f16<split>"; s.launch = L_conv0_valu<true>;
            s.grid = dim3(blocks_for((long)B * g.H * g.W, 256), 2);
        } else if (!sw.no_mfma0) {   // 416 = 26 x 16 = 13 x 32: the tile grid is exact
            s.kernel = "k_conv0_pool_mfma"; s.launch = L_conv0_mfma<false>;
            s.T = B * (416 / 16) * (416 / 32);
            s.grid = dim3((unsigned)std::min(s.T, 256 * Y2_CONV0_WGS));   // persistent workgroups, Y2_CONV0_WGS per CU
        } else {
            s.kernel = "k_conv0_pool_f16"; s.launch = L_conv0_valu<false>;
            s.grid = dim3(blocks_for((long)B * g.H * g.W, 256), 2);
        }
        if (g.B != B || g.H != 208 || g.W != 208 || g.Cp != (split ? 128 : 32)) return fail(YOLO2_ERROR, "fp16 plan: layer-1 tensor has the wrong geometry");
        P.steps.push_back(s);
        if (!sw.no_mfma0) {   // the same tiles, grid and output from image bytes (the images entries)
            P.u8 = s;
            P.u8.kernel = split ? "k_conv0_pool_mfma_u8<split>" : "k_conv0_pool_mfma_u8";
            P.launch_u8 = split ? L_conv0_mfma_u8<true> : L_conv0_mfma_u8<false>;
            P.yuyv_kernel = split ? "k_conv0_pool_mfma_yuyv<split>" : "k_conv0_pool_mfma_yuyv";
            P.launch_yuyv = split ? L_conv0_mfma_yuyv<true> : L_conv0_mfma_yuyv<false>;
        }
    }
    int ord = 1, skip_pool = -1, fused_conv = -1;
    const HT *cur = &c->h_out[1];
    for (int i = 2; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        switch (l.type) {
        case L_CONV: {
            if (i == fused_conv) {   // this 1x1 layer ran inside the launch of the 3x3 before it (k_conv_f16_rw MODE 2): its tensor exists already
                ord++;
                cur = &c->h_out[i];
                break;
            }
            const HT *tin = i == 26 ? &c->h_out[16] : (i == 29 ? &c->h_cat : cur);
            const HT &tout = c->h_out[i];
            F16Step s;
            s.layer = i; s.B = B;
            ConvF16Args &a = s.a;
            a.B = B; a.H = l.h; a.W = l.w; a.Wp = l.w + 1; a.PL = (l.h + 1) * (l.w + 1);
            a.Cp_in = tin->Cp;
            a.Cp_out = i == 30 ? 0 : tout.Cp;
            a.N = l.n;
            a.out_ch_off = i == 24 ? 256 : 0;
            a.n_store = i == 30 ? l.n : round_up(l.n, 32);
            a.npix = B * l.h * l.w;
            a.leaky = l.leaky;
            a.KS = l.size;
            a.pool = 0; a.oWp = a.oPL = a.npool = 0;
            a.n_tiles = 1;
            a.split_n = split && i != 30 ? part_stride(i == 24 ? 1280 : l.n) : 0;
            set_fast_div(a);
            a.stamp = sw.stamp_layer == i;
            s.w = (const _Float16 *)(c->wh + c->wh_off[ord]);
            s.bias = (const float *)(c->biasf + c->biasf_off[ord]);
            s.in = (const _Float16 *)tin->d;
            s.out = i == 30 ? (_Float16 *)nullptr : tout.d;
            s.store = i == 30 ? FS_REGION : FS_FULL_OR_POOL;
            const HT *dst = &tout;
            ord++;
            const bool bk64 = a.Cp_in % 64 == 0;   // K-step of 64 channels wherever the item size allows it
            const bool glds = bk64 && !sw.no_glds;   // LDS-DMA staging wherever the K-step is 64
            // Conv layers whose only consumer is the 2x2 pool after them (2 and 6; 10 runs the halo kernel, 16 also
            // feeds the route) store the pooled tensor directly: MFMA rows ordered by pool window, max in the epilogue.
            // The persistent halo kernel takes the 104x104 layers EXCEPT layer 6: it stores the full-resolution tensor only
            // (FS_FULL), and the pool kernel that then has to follow (0.08 ms at batch 128) costs more than the conv gains.
            const bool pool_next = kNet[i + 1].type == L_MAX && !sw.no_poolfuse;
            const bool persist_ok = !sw.no_glds && !sw.no_halo && !sw.no_persist && ((l.w > 52 && !(i == 6 && pool_next)) || sw.persist_all);
            const bool fuse_pool = (i == 2 || (i == 6 && !persist_ok)) && pool_next;
            if (fuse_pool) {
                const HT &tp = c->h_out[i + 1];
                a.pool = 1; a.oWp = tp.Wp; a.oPL = tp.PL; a.npool = B * tp.H * tp.W;
                a.Cp_out = tp.Cp;
                s.out = tp.d;
                dst = &tp;
                skip_pool = i + 1;
            }
            const bool in32 = ((size_t)kLead + (size_t)B * a.PL) * a.Cp_in * 2 < (1ull << 32);   // 32-bit byte offsets into the input
            int rc = YOLO2_SUCCESS;
            bool done = false;
            // The 64 -> 128 channel 3x3 layers at 104 x 104 (4 and 6): weights resident in registers, two image rows per tile, one barrier
            // per tile (k_conv_f16_rw).  Layer 6 fuses its pool (MODE 1); layer 4 fuses the 1x1 layer 5, its only consumer (MODE 2:
            // the 128-channel tensor between them is never written); MODE 0 stores the plain tensor.
            if (!done && !split && !sw.no_rw && l.size == 3 && a.Cp_in == 64 && l.n == 128 && l.w == 8 * 13 && (l.h & 1) == 0 && !sw.no_glds &&
                ((size_t)kLead + (size_t)B * a.PL + kTail) * 128 < (1ull << 31)) {   // (signed 32-bit byte offsets into the input)
                const bool pool_here = kNet[i + 1].type == L_MAX && !sw.no_poolfuse;
                const LayerDesc &nx = kNet[i + 1];
                const bool fuse1 = !pool_here && !sw.no_fuse1x1 && nx.type == L_CONV && nx.size == 1 && nx.c == 128 && nx.n == 64 && nx.leaky == l.leaky &&
                                   nx.h == l.h && nx.w == l.w && i + 1 != 16 && i + 1 != 24;   // (and nothing but layer i + 1 reads layer i: true for every conv of this network except 16)
                s.T = B * (l.h / 2);
                const int rounds = (s.T + 255) / 256;
                s.grid = dim3(std::min(256, std::max(8, round_up((s.T + rounds - 1) / rounds, 8)))); s.block = dim3(256);
                const int n_stage = (2 * l.w + 2 * (l.w + 1) + 7) / 8;
                const bool rwb_ok = !sw.no_rwb && l.leaky && a.n_store == 128;   // k_conv_f16_rwb: leaky layers, every channel stored
                if (pool_here) {
                    const HT &tp = c->h_out[i + 1];
                    a.pool = 1; a.oWp = tp.Wp; a.oPL = tp.PL; a.npool = B * tp.H * tp.W;
                    a.Cp_out = tp.Cp;
                    s.out = tp.d; dst = &tp; skip_pool = i + 1;
                    s.lt_rows = n_stage * 8;
                    s.lds = (unsigned)(2 * s.lt_rows * 128 + 13 * 1024 + 2 * (26 * 16 / 4 / 2) * 136 * 2);   // two input tiles + zero region + two pooled tiles
                    s.kernel = "k_conv_f16_rw<pool>"; s.launch = L_rw<1>; s.store = FS_POOL_ONLY;
                    if (rwb_ok) {       // the epilogue inside the MFMA stream (k_conv_f16_rwb)
                        s.lt_rows = 432;
                        s.lds = (unsigned)(2 * 432 * 128 + 2 * 52 * 136 * 2);
                        s.kernel = "k_conv_f16_rwb<pool>"; s.launch = L_rwb<1>;
                    }
                } else if (fuse1) {
                    const HT &t2 = c->h_out[i + 1];
                    a.Cp_out = t2.Cp; a.N = nx.n; a.n_store = round_up(nx.n, 32); a.out_ch_off = 0;
                    s.out = t2.d; dst = &t2; fused_conv = i + 1;
                    s.w2 = (const _Float16 *)(c->wh + c->wh_off[ord]);          // (ord was advanced above: the NEXT conv's weights)
                    s.bias2 = (const float *)(c->biasf + c->biasf_off[ord]);
                    s.lt_rows = std::max(n_stage, ((13 * 16 * 136 * 2 + 127) / 128 + 7) / 8) * 8;   // the 208 x 136-half intermediate tile must fit an input buffer
                    s.lds = (unsigned)(2 * s.lt_rows * 128 + 13 * 1024);
                    s.kernel = "k_conv_f16_rw<+1x1>"; s.launch = L_rw<2>; s.store = FS_FULL;
                    if (rwb_ok && nx.leaky && t2.Cp == 64) {
                        s.lt_rows = 432;
                        s.lds = (unsigned)(2 * 432 * 128 + 208 * 256);        // = 160 KB: the whole LDS of a CU
                        s.kernel = "k_conv_f16_rwb<+1x1>"; s.launch = L_rwb<2>;
                    }
                } else {
                    s.lt_rows = n_stage * 8;
                    s.lds = (unsigned)(2 * s.lt_rows * 128 + 13 * 1024);
                    s.kernel = "k_conv_f16_rw"; s.launch = L_rw<0>; s.store = FS_FULL;
                }
                done = true;
            }
            // 1x1 layers: persistent workgroups over a ring of staged K-steps (k_gemm1_f16_p)
            if (split && !bk64) return fail(YOLO2_ERROR, "fp16 plan (split): layer %d has %d-channel items, not a multiple of the 64-channel K-step", i, a.Cp_in);
            // 1x1 layers whose channel count is a multiple of 256 (13, 15: 256; 19, 21: 512): 128 pixels x 256 channels per tile, so that the
            // input - the bytes this HBM-bound layer moves - is read once per 256 output channels instead of once per 128
            // (experiment f16_ring_sq) the same layers on 256 x 256 tiles, sixteen wavefronts, two 64-KB stages: twice the FLOPs per staged byte of the
            // 128 x 128 tiles (an LDS-DMA'd byte feeds 128 FLOPs instead of 64), at the price of 338 / 170 tiles for 256 CUs
            if (!done && !split && sw.ring_sq && l.size == 1 && bk64 && i != 30 && l.n % 256 == 0 && in32 && !sw.no_ring) {
                a.n_tiles = l.n / 256;
                s.T = ((a.npix + 255) / 256) * a.n_tiles;
                const int rounds = (s.T + 255) / 256;
                s.grid = dim3(std::min(256, std::max(8, round_up((s.T + rounds - 1) / rounds, 8))));
                s.kernel = "k_gemm1_f16_p<256,256,2>"; s.launch = L_ring_sq; s.block = dim3(1024); s.lds = 2 * (256 + 256) * 128;
                s.store = FS_FULL;
                done = true;
            }
            if (!done && !split && sw.ring256 && l.size == 1 && bk64 && i != 30 && l.n % 256 == 0 && in32 && !sw.no_ring) {
                a.n_tiles = l.n / 256;
                s.T = ((a.npix + 127) / 128) * a.n_tiles;
                const int rounds = (s.T + 255) / 256;
                s.grid = dim3(std::min(256, std::max(8, round_up((s.T + rounds - 1) / rounds, 8))));
                s.kernel = "k_gemm1_f16_p<128,256,3>"; s.launch = L_ring256; s.block = dim3(512); s.lds = 3 * (128 + 256) * 128;
                s.store = FS_FULL;
                done = true;
            }
            if (!done && l.size == 1 && bk64 && (i == 30 || (sw.ring_all && !split)) && in32 && !sw.no_ring) {
                const int bn = l.n <= 64 ? 64 : 128;
                a.n_tiles = round_up(l.n, bn) / bn;
                s.T = ((a.npix + 255) / 256) * a.n_tiles;
                const int rounds = (s.T + 255) / 256;                                    // tiles per workgroup
                s.grid = dim3(std::min(256, std::max(8, round_up((s.T + rounds - 1) / rounds, 8))));
                if (bn == 64) { s.kernel = "k_gemm1_f16_p<256,64,3>"; s.launch = L_ring<64>; s.block = dim3(256); s.lds = 3 * (256 + 64) * 128; }
                else { s.kernel = "k_gemm1_f16_p<256,128,3>"; s.launch = L_ring<128>; s.block = dim3(512); s.lds = 3 * (256 + 128) * 128; }
                if (s.store != FS_REGION) s.store = FS_FULL;
                done = true;
            }
            // the 32-channel layer + its pool with the weights in registers and a ring of image rows in LDS (k_conv_f16_rwc): runs of
            // 52, 26 or 13 consecutive row pairs per workgroup - the longest that still gives every CU a run
            if (!done && !split && !sw.no_rwc && fuse_pool && a.Cp_in == 32 && l.size == 3 && l.n == 64 && l.w == 208 && l.h == 208 && l.leaky &&
                a.Cp_out == 64 && a.n_store == 64 && a.out_ch_off == 0 && ((size_t)kLead + (size_t)B * a.PL + kTail) * 64 < (1ull << 31)) {
                int run_len = 52;
                while (run_len > 13 && B * (l.h / 2 / run_len) < 256) run_len /= 2;
                s.lt_rows = run_len;                       // (the launcher hands it to the kernel)
                s.T = B * (l.h / 2 / run_len);             // runs
                s.kernel = "k_conv_f16_rwc"; s.launch = L_rwc; s.store = FS_POOL_ONLY;
                s.grid = dim3((unsigned)std::min(s.T, 256)); s.block = dim3(256);
                s.lds = (unsigned)(8 * 212 * 64 + 3 * 104 * 72 * 2);
                done = true;
            }
            // the 32-channel layer + its pool: 16 x 16 tiles, patch and all nine taps' weights resident in LDS (k_conv_f16_c32_pool)
            if (!done && fuse_pool && a.Cp_in == 32 && l.size == 3 && l.n == 64 && l.h % 16 == 0 && l.w % 16 == 0 && a.Cp_out >= 64 &&
                ((size_t)kLead + (size_t)B * a.PL) * 64 < (1ull << 32) && !sw.no_c32) {
                s.T = B * (l.h / 16) * (l.w / 16);
                s.kernel = "k_conv_f16_c32_pool"; s.launch = L_c32_pool; s.store = FS_POOL_ONLY;
                s.grid = dim3((unsigned)std::min(s.T, 512)); s.block = dim3(256); s.lds = (9 * 64 + 336) * 64;   // two workgroups per CU, weights staged once each
                done = true;
            }
            const int m_tiles = fuse_pool ? (a.npool + 31) / 32 : (a.npix + 127) / 128;   // 128-row tiles (32 pool windows)
            if (!done && l.n <= 64) {
                a.n_tiles = round_up(l.n, 64) / 64;
                s.grid = dim3(m_tiles * a.n_tiles); s.block = dim3(256);
                if (split) { s.kernel = "k_conv_f16_glds<64,split>"; s.launch = L_glds<64, true>; }
                else if (glds) { s.kernel = "k_conv_f16_glds<64>"; s.launch = L_glds<64>; }
                else if (bk64) { s.kernel = "k_conv_f16<128,64,64>"; s.launch = L_reg<64, 64>; }
                else { s.kernel = "k_conv_f16<128,64,32>"; s.launch = L_reg<64, 32>; }
                done = true;
            }
            if (!done) {
                a.n_tiles = round_up(l.n, kBN) / kBN;
                // dense halo tile: 256 pixels + W+1 on either side, rounded to 8-row groups, + 8 zero rows
                const int lt_rows = round_up(256 + 2 * (l.w + 1), 8) + 8;
                const size_t a_bytes = (size_t)2 * lt_rows * 128, cap = 160 * 1024;
                // persistent halo-tile kernel: the workgroup walks its tiles, the next tile's staging overlaps this one's tail
                if (glds && l.size == 3 && l.n % kBN == 0 && persist_ok && !fuse_pool) {
                    const bool off32 = ((size_t)kLead + (size_t)B * a.PL) * std::max(a.Cp_in, a.Cp_out) * 2 < (1ull << 32);
                    const bool wide = l.n % 256 == 0 && a_bytes + (size_t)2 * 256 * 128 <= cap;
                    const int bn = wide ? 256 : 128;
                    const size_t lds = a_bytes + (size_t)2 * bn * 128;
                    if (off32 && lds <= cap && lt_rows - 8 <= 8 * 8 * 8) {
                        a.n_tiles = l.n / bn;
                        s.T = ((a.npix + 255) / 256) * a.n_tiles;
                        const int rounds = (s.T + 255) / 256;
                        // (Launched with one tile per workgroup - the same kernel, only the LDS-free epilogue and the operand order
                        //  differ from k_conv_f16_halo - it measured 2.8 % slower over the pass at batch 256.)
                        s.grid = dim3(std::min(256, std::max(8, round_up((s.T + rounds - 1) / rounds, 8))));
                        s.lds = (unsigned)lds; s.lt_rows = lt_rows; s.store = FS_FULL;
                        if (split && wide) { s.kernel = "k_conv_f16_halo_p<256,16,32,split>"; s.launch = L_halo_p<256, 16, 32, true>; s.block = dim3(1024); }
                        else if (split) { s.kernel = "k_conv_f16_halo_p<128,8,32,split>"; s.launch = L_halo_p<128, 8, 32, true>; s.block = dim3(512); }
                        else if (wide && sw.m16) { s.kernel = "k_conv_f16_halo_p<256,16,16>"; s.launch = L_halo_p<256, 16, 16>; s.block = dim3(1024); }
                        else if (wide) { s.kernel = "k_conv_f16_halo_p<256,16,32>"; s.launch = L_halo_p<256, 16, 32>; s.block = dim3(1024); }
                        else if (sw.m16) { s.kernel = "k_conv_f16_halo_p<128,8,16>"; s.launch = L_halo_p<128, 8, 16>; s.block = dim3(512); }
                        else { s.kernel = "k_conv_f16_halo_p<128,8,32>"; s.launch = L_halo_p<128, 8, 32>; s.block = dim3(512); }
                        done = true;
                    }
                }
                // 3x3 layers: halo-tile kernel (input tile staged once per 64-channel chunk, nine taps read it
                // shifted) wherever its LDS arena fits: 2 x lt_rows x 128 B (A) + NB x BN x 128 B (B) + fo table
                if (!done && glds && l.size == 3 && l.n % kBN == 0 && !sw.no_halo && !fuse_pool) {
                    const size_t fo_bytes = 256 * sizeof(int);
                    const size_t lds256 = a_bytes + (size_t)2 * 256 * 128 + fo_bytes, lds128 = a_bytes + (size_t)3 * 128 * 128 + fo_bytes;
                    const bool wide = l.n % 256 == 0 && lds256 <= cap && a_bytes + (size_t)2 * 256 * 128 >= (size_t)256 * 264 * 2 && !sw.no_wide;
                    const bool three = lds128 <= cap;
                    // (the two-buffer 256x128 form that would fit the 104x104 layers runs one workgroup per CU and measured
                    //  6 % slower there than the 128x128 kernel with two: only the shapes below are used)
                    const bool fits = lt_rows - 8 <= 8 * 8 * 8 && a_bytes >= (size_t)256 * kCtRow * 2 && (wide || three) && in32;
                    if (fits) {   // (the kernels' dynamic-LDS limit was raised for this device in load_weights_fp32)
                        s.lt_rows = lt_rows; s.store = FS_FULL;
                        if (wide) {
                            a.n_tiles = l.n / 256;
                            s.grid = dim3(((a.npix + 255) / 256) * a.n_tiles); s.lds = (unsigned)lds256;
                            // a 256-channel 3x3 whose only consumer is a 1x1 down to 128 channels (layer 8 -> 9): the 1x1 runs in the epilogue
                            const LayerDesc &nx = kNet[i + 1];
                            const bool fuse1 = !split && !sw.no_fuse1x1 && !sw.m16 && !sw.w8 && l.n == 256 && a.n_tiles == 1 && nx.type == L_CONV && nx.size == 1 &&
                                               nx.c == 256 && nx.n == 128 && nx.leaky == l.leaky && nx.h == l.h && nx.w == l.w && i != 16 && i != 24;
                            if (fuse1) {
                                const HT &t2 = c->h_out[i + 1];
                                a.Cp_out = t2.Cp; a.N = nx.n; a.n_store = round_up(nx.n, 32); a.out_ch_off = 0;
                                s.out = t2.d; dst = &t2; fused_conv = i + 1;
                                s.w2 = (const _Float16 *)(c->wh + c->wh_off[ord]);          // (ord was advanced above: the NEXT conv's weights)
                                s.bias2 = (const float *)(c->biasf + c->biasf_off[ord]);
                                s.kernel = "k_conv_f16_halo<256,2,16>+1x1"; s.launch = L_halo<256, 2, 16, 32, false, true>; s.block = dim3(1024);
                            } else
                            if (split) { s.kernel = "k_conv_f16_halo<256,2,16,32,split>"; s.launch = L_halo<256, 2, 16, 32, true>; s.block = dim3(1024); }
                            else if (sw.m16) { s.kernel = "k_conv_f16_halo<256,2,16,16>"; s.launch = L_halo<256, 2, 16, 16>; s.block = dim3(1024); }
                            else if (!sw.w8) { s.kernel = "k_conv_f16_halo<256,2,16>"; s.launch = L_halo<256, 2, 16, 32>; s.block = dim3(1024); }   // 16 wavefronts of 64x64 (4 per SIMD, +4 %) instead of 8 of 128x64
                            else { s.kernel = "k_conv_f16_halo<256,2>"; s.launch = L_halo<256, 2, 8, 32>; s.block = dim3(512); }
                        } else {   // `fits` without `wide` implies `three`
                            s.grid = dim3(((a.npix + 255) / 256) * a.n_tiles); s.lds = (unsigned)lds128;
                            if (split) { s.kernel = "k_conv_f16_halo<128,3,8,32,split>"; s.launch = L_halo<128, 3, 8, 32, true>; }
                            else { s.kernel = "k_conv_f16_halo<128,3>"; s.launch = L_halo<128, 3, 8, 32>; }
                            s.block = dim3(512);
                        }
                        done = true;
                    }
                }
                // (a 256x128 tile with 8 wavefronts and per-tap A staging was measured 8 % SLOWER than 128x128
                //  with two workgroups per CU: without the halo reuse the bigger tile only adds barrier cost)
                if (!done) {
                    s.grid = dim3(m_tiles * a.n_tiles); s.block = dim3(256);
                    if (split) { s.kernel = "k_conv_f16_glds<128,split>"; s.launch = L_glds<128, true>; }
                    else if (glds) { s.kernel = "k_conv_f16_glds<128>"; s.launch = L_glds<128>; }
                    else if (bk64) { s.kernel = "k_conv_f16<128,128,64>"; s.launch = L_reg<128, 64>; }
                    else { s.kernel = "k_conv_f16<128,128,32>"; s.launch = L_reg<128, 32>; }
                    done = true;
                }
            }
            if ((rc = checked_push(s, *dst))) return rc;
            if (i != 30) cur = dst;
            break;
        }
        case L_MAX: {
            if (i == skip_pool) { cur = &c->h_out[i]; break; }   // already produced by the conv before it
            const HT &gi = *cur, &go = c->h_out[i];
            if (gi.B != B || go.B != B || gi.H != 2 * go.H || gi.W != 2 * go.W || gi.Cp != go.Cp)
                return fail(YOLO2_ERROR, "fp16 plan: pool layer %d: %d x %d x %d -> %d x %d x %d does not halve", i, gi.H, gi.W, gi.Cp, go.H, go.W, go.Cp);
            F16Step s;
            s.layer = i; s.B = B; s.kernel = "k_maxpool2_f16"; s.launch = L_maxpool;
            s.in = gi.d; s.out = go.d; s.oCp = go.Cp; s.OH = go.H; s.OW = go.W; s.iWp = gi.Wp; s.iPL = gi.PL; s.oWp = go.Wp; s.oPL = go.PL;
            s.grid = dim3(blocks_for((long)B * go.H * go.W * (go.Cp / 8), 256)); s.block = dim3(256);
            if (split) {
                s.kernel = "k_maxpool2_split"; s.launch = L_maxpool_split; s.oPS = part_stride(go.C);
                s.grid = dim3(blocks_for((long)B * go.H * go.W * (s.oPS / 8), 256));
            }
            P.steps.push_back(s);
            cur = &c->h_out[i];
            break;
        }
        case L_REORG: {
            const HT &gi = *cur, &go = c->h_cat;
            if (gi.B != B || go.B != B || gi.H != 26 || gi.W != 26 || gi.Cp < 64 || go.H != 13 || go.W != 13 || go.Cp < 256)
                return fail(YOLO2_ERROR, "fp16 plan: reorg layer %d has the wrong geometry", i);
            F16Step s;
            s.layer = i; s.B = B; s.kernel = "k_reorg_f16"; s.launch = L_reorg;
            s.in = gi.d; s.out = go.d; s.iCp = gi.Cp; s.iWp = gi.Wp; s.iPL = gi.PL; s.oCp = go.Cp; s.oWp = go.Wp; s.oPL = go.PL;
            if (split) { s.kernel = "k_reorg_split"; s.launch = L_reorg_split; s.iPS = part_stride(gi.C); s.oPS = part_stride(go.C); }
            s.grid = dim3(blocks_for((long)B * (split ? 3 * 128 : 128) * 169, 256)); s.block = dim3(256);   // one thread per channel pair (and part)
            P.steps.push_back(s);
            cur = &c->h_cat;
            break;
        }
        default:
            break;  // route: concat by placement; region: the last conv already wrote the dense fp32 tensor
        }
    }
    if (sw.skip) {   // diagnostic only: drop launches from the table (wrong results), to price them inside the overlapped step
        std::vector<F16Step> kept;
        for (const F16Step &s : P.steps) {
            const LayerDesc &l = kNet[s.layer];
            bool drop = false;
            if ((sw.skip & 1) && (s.layer == 5 || s.layer == 9)) drop = true;
            if ((sw.skip & 2) && s.layer == 0) drop = true;
            if ((sw.skip & 4) && (s.layer == 2 || s.layer == 4 || s.layer == 6)) drop = true;
            if ((sw.skip & 8) && (l.type == L_MAX || l.type == L_REORG)) drop = true;
            if ((sw.skip & 16) && l.type == L_CONV && l.size == 1 && s.layer != 5 && s.layer != 9) drop = true;
            if ((sw.skip & 32) && l.type == L_CONV && l.size == 3 && l.w == 13) drop = true;
            if (!drop) kept.push_back(s);
        }
        P.steps = kept;
    }
    P.batch = B;
    if (sw.verbose)   // (plan construction, not the launch path)
        for (const F16Step &s : P.steps)
            fprintf(stderr, "[yolo2_hip] fp16 plan B=%d L%-2d %-30s grid %u block %u lds %u\n", B, s.layer, s.kernel, s.grid.x, s.block.x, s.lds);
    return YOLO2_SUCCESS;
}

// Kernel chosen for layer `layer_idx` by the current fp16 plan (after the first run_batch_fp16 at this batch); "" if none.
extern "C" const char *yolo2_hip_fp16_layer_kernel(yolo2_hip_ctx *c, int layer_idx)
{
    if (!c) return "";
    if (!c->f16_lanes.empty()) c = c->f16_lanes[0];
    if (!c->f16_plan) return "";
    for (const F16Step &s : c->f16_plan->steps)
        if (s.layer == layer_idx) return s.kernel;
    return "";
}

// Number of part-batch lanes the fp16 pass uses from batch 64 (default 2; 1 = none).  A measurement knob that is part of the ABI:
// bench.py times the dominant kernel's launches ALONE (lanes = 1 at one lane's batch) for its per-kernel roofline object.
extern "C" int yolo2_hip_set_fp16_lanes(yolo2_hip_ctx *c, int lanes)
{
    if (!c || !c->f16_plan) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    if (lanes < 1 || lanes > 8) return fail(YOLO2_ERROR, "fp16 lanes: %d out of range (1..8)", lanes);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    c->f16_plan->sw.lanes = lanes;
    for (yolo2_hip_ctx *l : c->f16_lanes) yolo2_hip_destroy(l);    // rebuilt at the next run if still wanted
    c->f16_lanes.clear();
    return YOLO2_SUCCESS;
}

static int make_f16_lanes(yolo2_hip_ctx *c, int want_lanes)
{
    for (yolo2_hip_ctx *l : c->f16_lanes) yolo2_hip_destroy(l);
    c->f16_lanes.clear();
    if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming), YOLO2_ERROR);
    std::vector<yolo2_hip_ctx *> made;   // committed only when all lanes are complete
    bool ok = true;
    for (int i = 0; i < want_lanes && ok; ++i) {
        yolo2_hip_ctx *l = new (std::nothrow) yolo2_hip_ctx();
        if (!l) { ok = false; break; }
        made.push_back(l);
        l->device = c->device;
        l->is_lane = true;
        l->opt = c->opt;
        l->split = c->split;
        l->wh = c->wh; l->biasf = c->biasf; l->w0f = c->w0f;
        memcpy(l->wh_off, c->wh_off, sizeof(c->wh_off));
        memcpy(l->biasf_off, c->biasf_off, sizeof(c->biasf_off));
        l->f16_loaded = true;
        l->f16_plan = new (std::nothrow) F16Plan();
        ok = l->f16_plan && ((i == 0 && !y2_lane0_own_stream()) || (y2_lane_stream_create(&l->lane_stream) == YOLO2_SUCCESS &&
                                                                     hipEventCreateWithFlags(&l->ev_join, hipEventDisableTiming) == hipSuccess));
        if (ok) l->f16_plan->sw = c->f16_plan->sw;   // a lane runs the parent's kernel selection
    }
    if (!ok) {
        for (yolo2_hip_ctx *l : made) yolo2_hip_destroy(l);
        return fail(YOLO2_ERROR, "fp16 lanes: context / stream / event creation failed");
    }
    c->f16_lanes = made;
    if (c->prof) (void)yolo2_hip_set_profiling(c->f16_lanes[0], 1);
    return YOLO2_SUCCESS;
}

// The pass.  lb == nullptr: layer 0 reads the float frames at frames_dev (the table as it is).  lb != nullptr (the images entries):
// layer 0 reads frames lb_first .. lb_first + batch - 1 of the chunk staging buffer lb through the table's step "from bytes", or,
// for a chunk of YUYV frames (yuyv), "from YUYV bytes".
static int run_f16(yolo2_hip_ctx *c, uint64_t frames_dev, const uint8_t *lb, int lb_first, bool yuyv, int batch, uint64_t region_dev,
                   void *stream)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    if (!c->f16_loaded || !c->f16_plan) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    if ((!lb && !frames_dev) || !region_dev) return fail(YOLO2_ERROR, "null buffer address");
    if (batch <= 0 || batch > 4096) return fail(YOLO2_ERROR, "batch %d out of range", batch);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    hipStream_t st = (hipStream_t)stream;
    // Two half-batch lanes like the int16 path: the big-tile kernels run one workgroup per CU and a layer is only
    // 2-3 generations of workgroups, so a second stream's launches fill the last, partly empty generation.
    const int want_lanes = c->f16_plan->sw.lanes;
    if (!c->is_lane && batch >= 64 && want_lanes > 1 && batch % want_lanes == 0) {
        if ((int)c->f16_lanes.size() != want_lanes) {
            const int rc = make_f16_lanes(c, want_lanes);
            if (rc) return rc;
        }
        const int half = batch / want_lanes;
        // lanes 1.. on their own streams, lane 0 on the caller's; joins after every lane is enqueued (see yolo2_hip_run_batch_int16)
        HIP_TRY(hipEventRecord(c->ev_fork, st), YOLO2_ERROR);
        for (int k = 0; k < want_lanes; ++k) {
            const int i = (k + 1) % want_lanes;
            yolo2_hip_ctx *l = c->f16_lanes[i];
            hipStream_t ls = l->lane_stream ? l->lane_stream : st;
            if (l->lane_stream) HIP_TRY(hipStreamWaitEvent(ls, c->ev_fork, 0), YOLO2_ERROR);
            const int rc = run_f16(l, lb ? 0 : frames_dev + (uint64_t)i * half * YOLO2_FRAME_ELEMS * sizeof(float), lb, lb_first + i * half, yuyv, half,
                                   region_dev + (uint64_t)i * half * YOLO2_REGION_ELEMS * sizeof(float), ls);
            if (rc) return rc;
            if (l->lane_stream) HIP_TRY(hipEventRecord(l->ev_join, ls), YOLO2_ERROR);
        }
        for (int i = 0; i < want_lanes; ++i)
            if (c->f16_lanes[i]->lane_stream) HIP_TRY(hipStreamWaitEvent(st, c->f16_lanes[i]->ev_join, 0), YOLO2_ERROR);
        c->f16_last_batch = batch; c->f16_last_laned = true;
        return YOLO2_SUCCESS;
    }
    int rc = ensure_f16_batch(c, batch);
    if (rc) return rc;
    if (c->f16_plan->batch != batch && (rc = build_f16_plan(c, batch))) return rc;
    c->f16_last_batch = batch; c->f16_last_laned = false;
    if (c->prof && (rc = y2_ensure_prof_events(c))) return rc;
    hipEvent_t *ev = c->prof ? c->ev[c->prof_runs % yolo2_hip_ctx::kProfSlots] : nullptr;
    // the table walk: hipEvent slot i opens layer i, slot i+1 closes it (layers 0+1 are one launch, booked to layer 0)
    const float *frames = (const float *)(uintptr_t)frames_dev;
    float *region = (float *)(uintptr_t)region_dev;
    int next_ev = 0;
    const F16Plan &P = *c->f16_plan;
    if (lb && !P.launch_u8) return fail(YOLO2_ERROR, "fp16 plan has no layer-0 step from bytes");
    const F16LaunchU8 from_bytes = yuyv ? P.launch_yuyv : P.launch_u8;
    for (const F16Step &s : P.steps) {
        if (ev) for (; next_ev <= s.layer; ++next_ev) (void)hipEventRecord(ev[next_ev], st);   // layers without a launch of their own
        if (lb && s.layer == 0)
            from_bytes(P.u8, lb, lb_first, st);
        else
            s.launch(s, frames, region, st);
        if (ev) { (void)hipEventRecord(ev[s.layer + 1], st); next_ev = s.layer + 2; }
    }
    if (ev) for (; next_ev <= 32; ++next_ev) (void)hipEventRecord(ev[next_ev], st);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    if (ev) c->prof_runs++;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_run_batch_fp16(yolo2_hip_ctx *c, uint64_t frames_dev, int batch, uint64_t region_dev, void *stream)
{
    return run_f16(c, frames_dev, nullptr, 0, false, batch, region_dev, stream);
}

// ---------------------------------------------------------------------------- split-fp16: the MFMA path inside the fp32 tolerance
//
// BASELINE.json's north star asks for the floating-point form "within 1e-3 box-coord tolerance for fp32" on the matrix cores.  The
// plain fp16 path misses that (activations and weights rounded to 11 bits: max box-coordinate error 5.8e-3); the exact fp32 path
// (yolo2_fp32.hip) is bit-identical but VALU-bound (1.4 k frames/s).  Here every fp32 value v travels as TWO halves,
// hi = fp16(v) and lo = fp16(v - hi) (22 significant bits), and a product a w is taken as a_hi w_hi + a_lo w_hi + a_hi w_lo on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation (the dropped a_lo w_lo term is 2^-22 relative).  No new contraction kernel: an
// item holds three parts [a_hi | a_lo | a_hi], the weights are packed [w_hi | w_hi | w_lo], and the fp16 kernels contract over
// the tripled channels as they are; only their epilogues differ (SPLIT instantiations: bias + leaky in fp32, then the (hi, lo)
// split and three stores; pools take the max of the fp32 values).  Layer 0 runs k_conv0_pool_mfma<true> (frame values and weights split
// inside the kernel, three MFMAs per product; its fp32 VALU form k_conv0_pool_f16<true> - fp32 frames x fp32 weights - under f16_no_mfma0).  The region layer's kernel writes fp32 as before.  3x the MFMA work and activation bytes of the fp16 path
// for ~1e-6 relative error: reference arithmetic hls/core/core_compute.cpp:121-172 is what the result is within tolerance of.
static int ensure_tol_twin(yolo2_hip_ctx *c)
{
    if (c->tol) return YOLO2_SUCCESS;
    yolo2_hip_ctx *t = new (std::nothrow) yolo2_hip_ctx();
    if (!t) return fail(YOLO2_ERROR, "out of host memory");
    t->device = c->device;
    t->opt = c->opt;
    t->split = true;
    t->w0f = c->w0f; t->wf32 = c->wf32; t->bf32 = c->bf32;
    int rc = pack_half_weights(t, c->wf32, c->bf32);
    if (rc == YOLO2_SUCCESS && hipDeviceSynchronize() != hipSuccess) rc = fail(YOLO2_ERROR, "split weight packing failed");
    if (rc) { yolo2_hip_destroy(t); return rc; }
    t->f16_loaded = true;
    if (c->prof) (void)yolo2_hip_set_profiling(t, 1);
    c->tol = t;
    return YOLO2_SUCCESS;
}

// Same contract as yolo2_hip_run_batch_fp16 (float frames in HBM -> dense fp32 region tensor [batch][425][13][13], enqueued on
// `stream`), computed in the split representation.  Needs yolo2_hip_load_weights_fp32.
extern "C" int yolo2_hip_run_batch_f32tol(yolo2_hip_ctx *c, uint64_t frames_dev, int batch, uint64_t region_dev, void *stream)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    if (!c->f16_loaded || !c->wf32) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    const int rc = ensure_tol_twin(c);
    if (rc) return rc;
    return yolo2_hip_run_batch_fp16(c->tol, frames_dev, batch, region_dev, stream);
}

extern "C" int yolo2_hip_run_batch_f32tol_host(yolo2_hip_ctx *c, const float *frames, int batch, float *region)
{
    return y2_run_batch_host(c, frames, batch, region, [&](uint64_t fd, uint64_t rd) { return yolo2_hip_run_batch_f32tol(c, fd, batch, rd, nullptr); });
}

// Kernel the split-mode table runs for layer `layer_idx` (after the first yolo2_hip_run_batch_f32tol at this batch); "" if none.
extern "C" const char *yolo2_hip_f32tol_layer_kernel(yolo2_hip_ctx *c, int layer_idx) { return c && c->tol ? yolo2_hip_fp16_layer_kernel(c->tol, layer_idx) : ""; }
extern "C" int yolo2_hip_num_lanes_f32tol(yolo2_hip_ctx *c) { return c && c->tol && !c->tol->f16_lanes.empty() ? (int)c->tol->f16_lanes.size() : 1; }

// Test hook: the raw items of one frame's plane of layer `layer_idx`'s tensor from the last run of the fp16 pass (split = 0) or of the
// split-fp16 twin (split = 1).  which = 0: the frame's PL = (H+1)(W+1) items; 1: the kLead items before plane 0; 2: the kTail items after
// the last plane (of the lane that holds the frame).  geom[8] = C, Cp, H, W, Wp, items copied, part stride (split items: [hi | lo | hi]
// parts of that many channels; plain items: Cp), channel offset of the layer inside the items (layer 24: 256 of the concat tensor).
// out == NULL: geometry only.  Only tensors that a step of the current table writes can be read: the others are never stored.
extern "C" int yolo2_hip_debug_f16_tensor(yolo2_hip_ctx *c, int split, int layer_idx, int frame, int which, uint16_t *out, size_t cap,
                                          int *geom)
{
    if (!c || !geom) return fail(YOLO2_ERROR, "null argument");
    if (split) {
        if (!c->tol) return fail(YOLO2_ERROR, "no split-fp16 run yet (yolo2_hip_run_batch_f32tol)");
        c = c->tol;
    }
    if (!c->f16_last_batch) return fail(YOLO2_ERROR, "no fp16 run yet");
    if (frame < 0 || frame >= c->f16_last_batch) return fail(YOLO2_ERROR, "frame %d outside the last batch of %d", frame, c->f16_last_batch);
    if (which < 0 || which > 2) return fail(YOLO2_ERROR, "bad item range %d", which);
    if (c->f16_last_laned) {   // frame -> lane exactly as yolo2_hip_run_batch_fp16 splits the batch
        if (c->f16_lanes.empty()) return fail(YOLO2_ERROR, "the lanes of the last fp16 run are gone (yolo2_hip_set_fp16_lanes)");
        const int half = c->f16_last_batch / (int)c->f16_lanes.size();
        yolo2_hip_ctx *l = c->f16_lanes[frame / half];
        if (l->f16_last_batch != half || l->f16_last_laned) return fail(YOLO2_ERROR, "fp16 lane state does not match the last run");
        return yolo2_hip_debug_f16_tensor(l, 0, layer_idx, frame % half, which, out, cap, geom);
    }
    if (layer_idx < 0 || layer_idx > 30) return fail(YOLO2_ERROR, "bad layer %d", layer_idx);
    if (layer_idx == 30) return fail(YOLO2_ERROR, "layer 30's output is the region tensor the run returns");
    const LayerDesc &l = kNet[layer_idx];
    if (l.type == L_ROUTE) return fail(YOLO2_ERROR, "route layer %d has no tensor of its own", layer_idx);
    if (!c->f16_plan || c->f16_plan->batch != c->f16_last_batch) return fail(YOLO2_ERROR, "no launch table for the last run");
    const bool cat = layer_idx == 24 || layer_idx == 27;
    const yolo2_hip_ctx::HalfTensor &t = cat ? c->h_cat : c->h_out[layer_idx];
    bool written = false;   // from the table itself: some step stores into this tensor (layer 24 / 27: the step of that layer)
    for (const F16Step &s : c->f16_plan->steps)
        if (t.d && s.out == t.d && (!cat || s.layer == layer_idx)) written = true;
    if (!written)
        return fail(YOLO2_ERROR, "layer %d's tensor is not written by the current fp16 plan (its launch is fused or it has none)", layer_idx);
    const int C = l.type == L_MAX ? l.c : (l.type == L_REORG ? 4 * l.c : l.n);
    const int ps = c->split ? part_stride(cat ? 1280 : C) : t.Cp;
    const int g[8] = {C, t.Cp, t.H, t.W, t.Wp, which == 0 ? t.PL : (which == 1 ? kLead : kTail), ps, layer_idx == 24 ? 256 : 0};
    memcpy(geom, g, sizeof(g));
    if (!out) return YOLO2_SUCCESS;
    const size_t n = (size_t)g[5] * t.Cp;
    if (cap < n) return fail(YOLO2_ERROR, "output buffer too small (%zu < %zu halves)", cap, n);
    const size_t first = which == 0 ? (size_t)kLead + (size_t)frame * t.PL : (which == 1 ? 0 : (size_t)kLead + (size_t)t.B * t.PL);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);   // (lanes run on streams of their own)
    HIP_TRY(hipMemcpy(out, t.d + first * t.Cp, n * 2, hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

#ifdef Y2_STAMPS
// diagnostic build only: the halo kernel's workgroup timeline of the launch selected by YOLO2_STAMP_LAYER
extern "C" int yolo2_hip_debug_stamps(unsigned long long *dst, int n_wg)
{
    if (n_wg > kStampWGs) n_wg = kStampWGs;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(y2_stamps), (size_t)n_wg * 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int yolo2_hip_run_batch_fp16_host(yolo2_hip_ctx *c, const float *frames, int batch, float *region)
{
    return y2_run_batch_host(c, frames, batch, region, [&](uint64_t fd, uint64_t rd) { return yolo2_hip_run_batch_fp16(c, fd, batch, rd, nullptr); });
}

// ---------------------------------------------------------------------------- the images entries' pass (yolo2_hip.hip)

int y2_f16_images_ctx(yolo2_hip_ctx *c, int split, yolo2_hip_ctx **run)
{
    if (split != 0 && split != 1) return fail(YOLO2_ERROR, "split must be 0 (fp16) or 1 (fp32 tolerance), not %d", split);
    if (!c->f16_loaded || !c->f16_plan || !c->wf32) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    if (split) {
        HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
        const int rc = ensure_tol_twin(c);
        if (rc) return rc;
    }
    *run = split ? c->tol : c;
    return YOLO2_SUCCESS;
}

bool y2_f16_images_fused(const yolo2_hip_ctx *run) { return !run->f16_plan->sw.no_mfma0; }

int y2_f16_run_images(yolo2_hip_ctx *run, const uint8_t *lb, bool yuyv, int batch, float *region_dev, hipStream_t st)
{
    if (!lb) return fail(YOLO2_ERROR, "null buffer address");
    return run_f16(run, 0, lb, 0, yuyv, batch, (uint64_t)(uintptr_t)region_dev, st);
}

const char *y2_f16_images_kernel(const yolo2_hip_ctx *run, bool yuyv)
{
    if (!run->f16_lanes.empty() && run->f16_last_laned) run = run->f16_lanes[0];
    if (!run->f16_plan || !run->f16_plan->launch_u8) return "";
    return yuyv ? run->f16_plan->yuyv_kernel : run->f16_plan->u8.kernel;
}
