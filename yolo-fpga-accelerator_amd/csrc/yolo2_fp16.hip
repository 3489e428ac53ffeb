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
#include "kernels_f16_pix.hpp"

using namespace y2;

// ---------------------------------------------------------------------------- the launch table
//
// Which kernel runs which layer is decided ONCE per (context, batch) and stored as a table of steps; a pass is a walk over
// that table (no environment look-ups, no selection logic on the launch path).  The A/B switches of the kernel families
// (options f16_* of the context, from YOLO2_F16_* at context creation or yolo2_hip_set_option: tests and tools/abenv.sh use
// them) are latched once, when the weights are loaded: the plan keeps its own copy of the context's Y2Options.
// SELECTION (select_f16_table) is a function of (options, split mode, batch) alone - no HIP call, no device pointer, every field but
// the addresses (yolo2_hip_f16_plan_describe prints it without a GPU); BINDING (bind_f16_step) fills the addresses from a context.

struct F16Step;
typedef void (*F16Launch)(const F16Step &, const float *frames, float *region, hipStream_t);
typedef void (*F16LaunchU8)(const F16Step &, const uint8_t *lb, int lb_first, hipStream_t);

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
    ConvF16Args a = {};
    dim3 grid, block;
    unsigned lds = 0;
    int lt_rows = 0, T = 0;      // extra kernel arguments (halo tile rows, persistent kernels' tile count)
    int B = 0;
    // pool / reorg steps: source and destination geometry (iPS / oPS: part strides of split items)
    int iCp = 0, iWp = 0, iPL = 0, oCp = 0, oWp = 0, oPL = 0, OH = 0, OW = 0, iPS = 0, oPS = 0;
    // What the step reads and writes as selection names it - tensors by the layer whose output they hold (f16_geom; -1: the caller's
    // frames / region buffer), weights by conv ordinal (-1: none; w2: the 1x1 layer fused behind a 3x3) - and as binding resolves it
    int t_in = -1, t_out = -1, w_ord = -1, w2_ord = -1;
    const _Float16 *in = nullptr, *w = nullptr, *w2 = nullptr;
    const float *bias = nullptr, *w0 = nullptr, *bias2 = nullptr;
    _Float16 *out = nullptr;
};

struct F16Table {
    int batch = 0;               // the batch the table below was built for (0 = none)
    std::vector<F16Step> steps;
    // the images entries' layer-0 step "from bytes" (layers 0+1 from a chunk's staging buffer), used instead of steps[0]; every
    // other step is the table's.  Not set (launch_u8 == nullptr) under f16_no_mfma0: those entries letterbox into frames first.
    // launch_pix / pix_kernel [Y2PixKind]: the same step from a chunk of frames of that kind (k_conv0_pool_mfma_yuyv / _nv12 / _i420 / _bgr24 / _rgba32 / _bgra32;
    // [Y2_KIND_BYTES] is launch_u8 / u8.kernel again).
    F16Step u8;
    F16LaunchU8 launch_u8 = nullptr, launch_pix[Y2_KIND_COUNT] = {};
    const char *pix_kernel[Y2_KIND_COUNT] = {"", "", "", "", "", "", ""};
};
struct F16Plan : F16Table {
    Y2Options opt;               // the context's option set as it was when the weights were loaded; a lane runs the parent's selection
    int lanes = 2;               // the only member that changes afterwards (yolo2_hip_set_fp16_lanes): f16_no_lanes ? 1 : f16_lanes
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
static int raise_f16_lds_limits();   // (walks the kernel registry below)

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
    for (int ord = 0; ord < YOLO2_N_CONV; ++ord) {
        const int i = kConvLayer[ord];
        const LayerDesc &l = kNet[i];
        const int npad = round_up(l.n, l.n <= 64 ? 64 : kBN);
        c->wh_off[ord] = wtot;
        c->biasf_off[ord] = btot;
        wtot += i == 0 ? (long)npad * 32 : (long)npad * l.size * l.size * item_halves(l.c, c->split);
        btot += npad;
    }
    for (yolo2_hip_ctx *l : c->f16_lanes) yolo2_hip_destroy(l);   // they alias the buffers that are about to be replaced
    c->f16_lanes.clear();
    y2_f16_plan_free(c);
    c->f16_plan = new (std::nothrow) F16Plan();
    if (!c->f16_plan) return fail(YOLO2_ERROR, "out of host memory");
    c->f16_plan->opt = c->opt;   // the ONLY place the fp16 path reads the context's switches
    c->f16_plan->lanes = c->opt.f16_no_lanes ? 1 : c->opt.f16_lanes;
    int rc;
    c->wh_own.reset();
    c->biasf_own.reset();
    c->wh = nullptr;
    c->biasf = nullptr;
    if ((rc = y2_alloc_owned(c->wh_own, c->wh, (size_t)wtot)) || (rc = y2_alloc_owned(c->biasf_own, c->biasf, (size_t)btot))) return rc;
    for (int ord = 0; ord < YOLO2_N_CONV; ++ord) {
        const int i = kConvLayer[ord];
        const LayerDesc &l = kNet[i];
        const long woff = kWire[i].w_off, boff = kWire[i].b_off;
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
    if ((rc = raise_f16_lds_limits())) return rc;
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

// ---- tensor geometry: follows from kNet, the batch and the split mode; nothing here allocates.  The tensor that holds layer i's
// output (NetWire's shape: a pool layer's is the pooled map, a member of the concat's the concat tensor it is placed in).  C == 0: the
// layer has none - layer 0's 416x416x32 tensor never exists (conv0+pool are fused), a route of one source is an alias, the last conv
// writes the region buffer.
typedef yolo2_hip_ctx::HalfGeom HalfGeom;
static HalfGeom f16_geom(int i, bool split, int B)
{
    HalfGeom g;
    if (i < 1 || kWire[i].to_region || !(kNet[i].type == L_CONV || kNet[i].type == L_MAX || kWire[i].cat >= 0)) return g;
    g.C = kWire[i].C; g.H = kWire[i].H; g.W = kWire[i].W;
    g.Cp = item_halves(g.C, split); g.Wp = g.W + 1; g.PL = (g.H + 1) * g.Wp; g.B = B;
    g.items = (size_t)kLead + (size_t)B * g.PL + kTail;
    return g;
}

static int alloc_half(yolo2_hip_ctx::HalfTensor &t, const HalfGeom &g)
{
    static_cast<HalfGeom &>(t) = g;
    const int rc = y2_alloc_owned(t.own, t.d, t.items * t.Cp);
    if (rc) return rc;
    HIP_TRY(hipMemset(t.d, 0, t.items * t.Cp * 2), YOLO2_DMA_ERROR);  // zeros = conv padding and channel padding
    return YOLO2_SUCCESS;
}

static int ensure_f16_batch(yolo2_hip_ctx *c, int B)
{
    if (c->f16_batch == B) return YOLO2_SUCCESS;
    y2_free_tensors(c->h_in, c->h_out, c->h_cat, c->f16_batch);
    if (c->f16_plan) { c->f16_plan->batch = 0; c->f16_plan->steps.clear(); }   // the table points into the tensors just freed
    int rc;
    if ((rc = y2_alloc_tensors(c->h_out, c->h_cat, [&](yolo2_hip_ctx::HalfTensor &t, int i) {
             const HalfGeom g = f16_geom(i, c->split, B);
             return g.C ? alloc_half(t, g) : (int)YOLO2_SUCCESS;
         })))
        return rc;
    c->f16_batch = B;
    // the zero fills above run on the null stream; the pass may be enqueued on a non-blocking stream (the lanes'
    // are), which does not order itself behind it
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// ---- launchers: one per kernel signature (K: the instantiation), all with the table's signature
#define Y2_LAUNCHER(name, ...)                                                                                        \
    template <auto K> static void name(const F16Step &s, const float *frames, float *region, hipStream_t st)        \
    { (void)frames; (void)region; hipLaunchKernelGGL(K, s.grid, s.block, s.lds, st, __VA_ARGS__); }
Y2_LAUNCHER(L_conv0_mfma, frames, s.w0, s.bias, s.out, 416, 416, s.oWp, s.oPL, s.T)
Y2_LAUNCHER(L_conv0_valu, frames, s.w0, s.bias, s.out, s.B, 416, 416, s.oWp, s.oPL)
Y2_LAUNCHER(L_gemm, s.in, s.w, s.bias, s.out, s.store == FS_REGION ? region : (float *)nullptr, s.a)         // k_conv_f16_glds, k_conv_f16
Y2_LAUNCHER(L_ring, s.in, s.w, s.bias, s.out, s.store == FS_REGION ? region : (float *)nullptr, s.a, s.T)    // k_gemm1_f16_p
Y2_LAUNCHER(L_tiles, s.in, s.w, s.bias, s.out, s.a, s.T)                                                       // k_conv_f16_c32_pool
Y2_LAUNCHER(L_rows, s.in, s.w, s.bias, s.out, s.a, s.lt_rows, s.T)                                             // k_conv_f16_rwc, k_conv_f16_halo_p
Y2_LAUNCHER(L_halo, s.in, s.w, s.bias, s.out, s.a, s.lt_rows, s.w2, s.bias2)
Y2_LAUNCHER(L_rw, s.in, s.w, s.bias, s.out, s.w2, s.bias2, s.a, s.lt_rows, s.T)
Y2_LAUNCHER(L_rwb, s.in, s.w, s.bias, s.out, s.w2, s.bias2, s.a, s.T)
Y2_LAUNCHER(L_maxpool_split, s.in, s.out, s.oPS, s.oCp, s.B, s.OH, s.OW, s.iWp, s.iPL, s.oWp, s.oPL)
Y2_LAUNCHER(L_maxpool, s.in, s.out, s.oCp, s.B, s.OH, s.OW, s.iWp, s.iPL, s.oWp, s.oPL)
Y2_LAUNCHER(L_reorg_split, s.in, s.out, s.B, s.iPS, s.iCp, s.iWp, s.iPL, s.oPS, s.oCp, s.oWp, s.oPL)
Y2_LAUNCHER(L_reorg, s.in, s.out, s.B, s.iCp, s.iWp, s.iPL, s.oCp, s.oWp, s.oPL)
#undef Y2_LAUNCHER
template <auto K> static void L_conv0_bytes(const F16Step &s, const uint8_t *lb, int lb_first, hipStream_t st)   // the images entries' layer 0
{
    hipLaunchKernelGGL(K, s.grid, s.block, 0, st, lb, lb_first, s.w0, s.bias, s.out, s.oWp, s.oPL, s.T);
}

// ---- the kernel registry: every instantiation the table can name, ONCE - its name string (tools, bench.py, the profiles and the
// tests key on these), its launcher and kernel, its block size and whether the kernel's dynamic-LDS limit is raised to the whole
// 160 KiB of a CU at weight load.  XB: the bytes form of layer 0.  A selection site names an entry (use()).
#define F16_KERNELS(X, XB)                                                                                             \
    X(FK_C0_MFMA_SP,     "k_conv0_pool_mfma<split>",           L_conv0_mfma, k_conv0_pool_mfma<true>, 256, 0)          \
    X(FK_C0_MFMA,        "k_conv0_pool_mfma",                  L_conv0_mfma, k_conv0_pool_mfma<false>, 256, 0)         \
    X(FK_C0_VALU_SP,     "k_conv0_pool_f16<split>",            L_conv0_valu, k_conv0_pool_f16<true>, 256, 0)           \
    X(FK_C0_VALU,        "k_conv0_pool_f16",                   L_conv0_valu, k_conv0_pool_f16<false>, 256, 0)          \
    XB(FK_C0_U8_SP,      "k_conv0_pool_mfma_u8<split>",        k_conv0_pool_mfma_u8<true>)                             \
    XB(FK_C0_U8,         "k_conv0_pool_mfma_u8",               k_conv0_pool_mfma_u8<false>)                            \
    XB(FK_C0_YUYV_SP,    "k_conv0_pool_mfma_yuyv<split>",      k_conv0_pool_mfma_yuyv<true>)                           \
    XB(FK_C0_YUYV,       "k_conv0_pool_mfma_yuyv",             k_conv0_pool_mfma_yuyv<false>)                          \
    XB(FK_C0_NV12_SP,    "k_conv0_pool_mfma_nv12<split>",      k_conv0_pool_mfma_nv12<true>)                           \
    XB(FK_C0_NV12,       "k_conv0_pool_mfma_nv12",             k_conv0_pool_mfma_nv12<false>)                          \
    XB(FK_C0_I420_SP,    "k_conv0_pool_mfma_i420<split>",      k_conv0_pool_mfma_i420<true>)                           \
    XB(FK_C0_I420,       "k_conv0_pool_mfma_i420",             k_conv0_pool_mfma_i420<false>)                          \
    X(FK_RW,             "k_conv_f16_rw",                      L_rw, (k_conv_f16_rw<13, 0>), 256, 1)                   \
    X(FK_RW_POOL,        "k_conv_f16_rw<pool>",                L_rw, (k_conv_f16_rw<13, 1>), 256, 1)                   \
    X(FK_RW_1X1,         "k_conv_f16_rw<+1x1>",                L_rw, (k_conv_f16_rw<13, 2>), 256, 1)                   \
    X(FK_RWB_POOL,       "k_conv_f16_rwb<pool>",               L_rwb, k_conv_f16_rwb<1>, 256, 1)                       \
    X(FK_RWB_1X1,        "k_conv_f16_rwb<+1x1>",               L_rwb, k_conv_f16_rwb<2>, 256, 1)                       \
    X(FK_RING_SQ,        "k_gemm1_f16_p<256,256,2>",           L_ring, (k_gemm1_f16_p<256, 256, 2>), 1024, 1)          \
    X(FK_RING256,        "k_gemm1_f16_p<128,256,3>",           L_ring, (k_gemm1_f16_p<128, 256, 3>), 512, 1)           \
    X(FK_RING_64,        "k_gemm1_f16_p<256,64,3>",            L_ring, (k_gemm1_f16_p<256, 64, 3>), 256, 1)            \
    X(FK_RING_128,       "k_gemm1_f16_p<256,128,3>",           L_ring, (k_gemm1_f16_p<256, 128, 3>), 512, 1)           \
    X(FK_RWC,            "k_conv_f16_rwc",                     L_rows, k_conv_f16_rwc, 256, 1)                         \
    X(FK_C32_POOL,       "k_conv_f16_c32_pool",                L_tiles, k_conv_f16_c32_pool, 256, 0)                   \
    X(FK_GLDS_64_SP,     "k_conv_f16_glds<64,split>",          L_gemm, (k_conv_f16_glds<64, true>), 256, 0)            \
    X(FK_GLDS_64,        "k_conv_f16_glds<64>",                L_gemm, (k_conv_f16_glds<64, false>), 256, 0)           \
    X(FK_REG_64_64,      "k_conv_f16<128,64,64>",              L_gemm, (k_conv_f16<128, 64, 64>), 256, 0)              \
    X(FK_REG_64_32,      "k_conv_f16<128,64,32>",              L_gemm, (k_conv_f16<128, 64, 32>), 256, 0)              \
    X(FK_GLDS_128_SP,    "k_conv_f16_glds<128,split>",         L_gemm, (k_conv_f16_glds<128, true>), 256, 0)           \
    X(FK_GLDS_128,       "k_conv_f16_glds<128>",               L_gemm, (k_conv_f16_glds<128, false>), 256, 0)          \
    X(FK_REG_128_64,     "k_conv_f16<128,128,64>",             L_gemm, (k_conv_f16<128, 128, 64>), 256, 0)             \
    X(FK_REG_128_32,     "k_conv_f16<128,128,32>",             L_gemm, (k_conv_f16<128, 128, 32>), 256, 0)             \
    X(FK_HALO_P_256_SP,  "k_conv_f16_halo_p<256,16,32,split>", L_rows, (k_conv_f16_halo_p<256, 16, 32, true>), 1024, 1) \
    X(FK_HALO_P_256_M16, "k_conv_f16_halo_p<256,16,16>",       L_rows, (k_conv_f16_halo_p<256, 16, 16, false>), 1024, 1) \
    X(FK_HALO_P_256,     "k_conv_f16_halo_p<256,16,32>",       L_rows, (k_conv_f16_halo_p<256, 16, 32, false>), 1024, 1) \
    X(FK_HALO_P_128_SP,  "k_conv_f16_halo_p<128,8,32,split>",  L_rows, (k_conv_f16_halo_p<128, 8, 32, true>), 512, 1)  \
    X(FK_HALO_P_128_M16, "k_conv_f16_halo_p<128,8,16>",        L_rows, (k_conv_f16_halo_p<128, 8, 16, false>), 512, 1) \
    X(FK_HALO_P_128,     "k_conv_f16_halo_p<128,8,32>",        L_rows, (k_conv_f16_halo_p<128, 8, 32, false>), 512, 1) \
    X(FK_HALO_256_1X1,   "k_conv_f16_halo<256,2,16>+1x1",      L_halo, (k_conv_f16_halo<256, 2, 16, 32, false, true>), 1024, 1) \
    X(FK_HALO_256_SP,    "k_conv_f16_halo<256,2,16,32,split>", L_halo, (k_conv_f16_halo<256, 2, 16, 32, true, false>), 1024, 1) \
    X(FK_HALO_256_M16,   "k_conv_f16_halo<256,2,16,16>",       L_halo, (k_conv_f16_halo<256, 2, 16, 16, false, false>), 1024, 1) \
    X(FK_HALO_256,       "k_conv_f16_halo<256,2,16>",          L_halo, (k_conv_f16_halo<256, 2, 16, 32, false, false>), 1024, 1) \
    X(FK_HALO_256_W8,    "k_conv_f16_halo<256,2>",             L_halo, (k_conv_f16_halo<256, 2, 8, 32, false, false>), 512, 1) \
    X(FK_HALO_128_SP,    "k_conv_f16_halo<128,3,8,32,split>",  L_halo, (k_conv_f16_halo<128, 3, 8, 32, true, false>), 512, 1) \
    X(FK_HALO_128,       "k_conv_f16_halo<128,3>",             L_halo, (k_conv_f16_halo<128, 3, 8, 32, false, false>), 512, 1) \
    X(FK_MAXPOOL_SP,     "k_maxpool2_split",                   L_maxpool_split, k_maxpool2_split, 256, 0)              \
    X(FK_MAXPOOL,        "k_maxpool2_f16",                     L_maxpool, k_maxpool2_f16, 256, 0)                      \
    X(FK_REORG_SP,       "k_reorg_split",                      L_reorg_split, k_reorg_split, 256, 0)                   \
    X(FK_REORG,          "k_reorg_f16",                        L_reorg, k_reorg_f16, 256, 0)                           \
    XB(FK_C0_BGR24_SP,   "k_conv0_pool_mfma_bgr24<split>",     k_conv0_pool_mfma_bgr24<true>)                          \
    XB(FK_C0_BGR24,      "k_conv0_pool_mfma_bgr24",            k_conv0_pool_mfma_bgr24<false>)                         \
    XB(FK_C0_RGBA32_SP,  "k_conv0_pool_mfma_rgba32<split>",    k_conv0_pool_mfma_rgba32<true>)                         \
    XB(FK_C0_RGBA32,     "k_conv0_pool_mfma_rgba32",           k_conv0_pool_mfma_rgba32<false>)                        \
    XB(FK_C0_BGRA32_SP,  "k_conv0_pool_mfma_bgra32<split>",    k_conv0_pool_mfma_bgra32<true>)                         \
    XB(FK_C0_BGRA32,     "k_conv0_pool_mfma_bgra32",           k_conv0_pool_mfma_bgra32<false>)
struct F16Kernel { const char *name; F16Launch launch; F16LaunchU8 launch_u8; unsigned block; const void *raise_lds; };
#define ID(id, ...) id,
enum F16Kid { F16_KERNELS(ID, ID) };
#define X(id, name, form, kernel, block, raise) {name, form<kernel>, nullptr, block, raise ? (const void *)kernel : nullptr},
#define XB(id, name, kernel) {name, nullptr, L_conv0_bytes<kernel>, 256, nullptr},
static const F16Kernel kF16Kernels[] = {F16_KERNELS(X, XB)};
#undef ID
#undef X
#undef XB

static int raise_f16_lds_limits()
{
    for (const F16Kernel &k : kF16Kernels)
        if (k.raise_lds) HIP_TRY(hipFuncSetAttribute(k.raise_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}
static void use(F16Step &s, F16Kid k) { s.kernel = kF16Kernels[k].name; s.launch = kF16Kernels[k].launch; s.block = dim3(kF16Kernels[k].block); }

// ---- selection: (options, split mode, batch) -> the table without addresses.  The rules are those measured in rounds 1-4 (DESIGN.md
// 4.3).  One function per kernel family, tried in the order of select_f16_table; each either takes the layer (fills the step, returns
// true) or declines it and leaves the step as it found it.
struct F16Conv {              // one conv layer as the family functions see it: none of them needs more than this and the step it fills
    const Y2Options &o;
    bool split;               // "fp32tol" mode: items of three parts [hi | lo | hi], SPLIT kernel instantiations
    int B, i;
    const LayerDesc &l;
    bool bk64, glds;          // K-step of 64 channels wherever the item size allows it; LDS-DMA staging wherever the K-step is 64
    bool pool_next, persist_ok, fuse_pool, in32;   // (in32: 32-bit byte offsets into the input)
};
constexpr size_t kLdsCap = 160 * 1024;
// persistent kernels: every workgroup walks the same number of tiles (`rounds`); a multiple of 8 workgroups, at most one per CU
static dim3 persistent_grid(int T)
{
    const int rounds = (T + 255) / 256;
    return dim3(std::min(256, std::max(8, round_up((T + rounds - 1) / rounds, 8))));
}
// the step stores the pooled tensor of layer i + 1 (which then has no launch of its own)
static void fuse_pool_into_next(const F16Conv &q, F16Step &s)
{
    const HalfGeom tp = f16_geom(q.i + 1, q.split, q.B);
    s.a.pool = 1; s.a.oWp = tp.Wp; s.a.oPL = tp.PL; s.a.npool = q.B * tp.H * tp.W; s.a.Cp_out = tp.Cp; s.t_out = q.i + 1;
}
// Layer i + 1 may run in layer i's epilogue: nothing else reads layer i (the tensor between them is never written), and layer
// i + 1's output starts at channel 0 of the tensor it lives in (true for every conv -> 1x1 pair of this network).
static bool next_is_only_reader(int i) { return kWire[i].readers == 1 && kWire[i + 1].src == i && kWire[i + 1].ch_off == 0; }
// the step runs the 1x1 layer i + 1 in its epilogue and stores THAT layer's tensor
static void fuse_1x1_next(const F16Conv &q, F16Step &s)
{
    const LayerDesc &nx = kNet[q.i + 1];
    s.a.Cp_out = f16_geom(q.i + 1, q.split, q.B).Cp; s.a.N = nx.n; s.a.n_store = round_up(nx.n, 32); s.a.out_ch_off = 0;
    s.t_out = q.i + 1; s.w2_ord = s.w_ord + 1;   // (the NEXT conv's weights)
}
// The 64 -> 128 channel 3x3 layers at 104 x 104 (4 and 6): weights resident in registers, two image rows per tile, one barrier
// per tile (k_conv_f16_rw).  Layer 6 fuses its pool (MODE 1); layer 4 fuses the 1x1 layer 5, its only consumer (MODE 2:
// the 128-channel tensor between them is never written); MODE 0 stores the plain tensor.
static bool take_rw(const F16Conv &q, F16Step &s)
{
    const LayerDesc &l = q.l, &nx = kNet[q.i + 1]; ConvF16Args &a = s.a;
    if (q.split || q.o.f16_no_rw || l.size != 3 || a.Cp_in != 64 || l.n != 128 || l.w != 8 * 13 || (l.h & 1) || q.o.f16_no_glds ||
        ((size_t)kLead + (size_t)q.B * a.PL + kTail) * 128 >= (1ull << 31))   // (signed 32-bit byte offsets into the input)
        return false;
    const bool fuse1 = !q.pool_next && !q.o.f16_no_fuse1x1 && nx.type == L_CONV && nx.size == 1 && nx.c == 128 && nx.n == 64 && nx.leaky == l.leaky &&
                       nx.h == l.h && nx.w == l.w && next_is_only_reader(q.i);
    s.T = q.B * (l.h / 2); s.grid = persistent_grid(s.T);
    const int n_stage = (2 * l.w + 2 * (l.w + 1) + 7) / 8;
    const bool rwb_ok = !q.o.f16_no_rwb && l.leaky && a.n_store == 128;   // k_conv_f16_rwb: leaky layers, every channel stored
    s.lt_rows = n_stage * 8;
    s.lds = (unsigned)(2 * s.lt_rows * 128 + 13 * 1024);   // two input tiles + zero region
    use(s, FK_RW); s.store = FS_FULL;
    if (q.pool_next) {
        fuse_pool_into_next(q, s);
        s.lds += 2 * (26 * 16 / 4 / 2) * 136 * 2;   // + two pooled tiles
        use(s, FK_RW_POOL); s.store = FS_POOL_ONLY;
        // the epilogue inside the MFMA stream (k_conv_f16_rwb)
        if (rwb_ok) { s.lt_rows = 432; s.lds = (unsigned)(2 * 432 * 128 + 2 * 52 * 136 * 2); use(s, FK_RWB_POOL); }
    } else if (fuse1) {
        fuse_1x1_next(q, s);
        s.lt_rows = std::max(n_stage, ((13 * 16 * 136 * 2 + 127) / 128 + 7) / 8) * 8;   // the 208 x 136-half intermediate tile must fit an input buffer
        s.lds = (unsigned)(2 * s.lt_rows * 128 + 13 * 1024); use(s, FK_RW_1X1);
        // (rwb: 2 x 432 x 128 + 208 x 256 = 160 KB: the whole LDS of a CU)
        if (rwb_ok && nx.leaky && a.Cp_out == 64) { s.lt_rows = 432; s.lds = (unsigned)(2 * 432 * 128 + 208 * 256); use(s, FK_RWB_1X1); }
    }
    return true;
}
// 1x1 layers: persistent workgroups over a ring of staged K-steps (k_gemm1_f16_p), bm pixels x bn channels per tile
static void ring_tiles(F16Step &s, int bm, int bn, F16Kid k, unsigned lds)
{
    s.a.n_tiles = round_up(s.a.N, bn) / bn;
    s.T = ((s.a.npix + bm - 1) / bm) * s.a.n_tiles; s.grid = persistent_grid(s.T);
    use(s, k); s.lds = lds; if (s.store != FS_REGION) s.store = FS_FULL;
}
static bool take_ring(const F16Conv &q, F16Step &s)
{
    if (q.l.size != 1 || !q.bk64 || !q.in32 || q.o.f16_no_ring) return false;
    // 1x1 layers whose channel count is a multiple of 256 (13, 15: 256; 19, 21: 512): 128 pixels x 256 channels per tile, so that the
    // input - the bytes this HBM-bound layer moves - is read once per 256 output channels instead of once per 128
    // (experiment f16_ring_sq) the same layers on 256 x 256 tiles, sixteen wavefronts, two 64-KB stages: twice the FLOPs per staged byte of the
    // 128 x 128 tiles (an LDS-DMA'd byte feeds 128 FLOPs instead of 64), at the price of 338 / 170 tiles for 256 CUs
    const bool n256 = !q.split && q.i != 30 && q.l.n % 256 == 0;
    if (n256 && q.o.f16_ring_sq) ring_tiles(s, 256, 256, FK_RING_SQ, 2 * (256 + 256) * 128);
    else if (n256 && q.o.f16_ring256) ring_tiles(s, 128, 256, FK_RING256, 3 * (128 + 256) * 128);
    else if (q.i != 30 && (!q.o.f16_ring_all || q.split)) return false;
    else if (q.l.n <= 64) ring_tiles(s, 256, 64, FK_RING_64, 3 * (256 + 64) * 128);
    else ring_tiles(s, 256, 128, FK_RING_128, 3 * (256 + 128) * 128);
    return true;
}
// the 32-channel layer + its pool with the weights in registers and a ring of image rows in LDS (k_conv_f16_rwc): runs of
// 52, 26 or 13 consecutive row pairs per workgroup - the longest that still gives every CU a run
static bool take_rwc(const F16Conv &q, F16Step &s)
{
    const LayerDesc &l = q.l; const ConvF16Args &a = s.a;
    if (q.split || q.o.f16_no_rwc || !q.fuse_pool || a.Cp_in != 32 || l.size != 3 || l.n != 64 || l.w != 208 || l.h != 208 || !l.leaky ||
        a.Cp_out != 64 || a.n_store != 64 || a.out_ch_off != 0 || ((size_t)kLead + (size_t)q.B * a.PL + kTail) * 64 >= (1ull << 31))
        return false;
    int run_len = 52;
    while (run_len > 13 && q.B * (l.h / 2 / run_len) < 256) run_len /= 2;
    s.lt_rows = run_len;                       // (the launcher hands it to the kernel)
    s.T = q.B * (l.h / 2 / run_len);           // runs
    use(s, FK_RWC); s.store = FS_POOL_ONLY;
    s.grid = dim3((unsigned)std::min(s.T, 256)); s.lds = (unsigned)(8 * 212 * 64 + 3 * 104 * 72 * 2);
    return true;
}
// the 32-channel layer + its pool: 16 x 16 tiles, patch and all nine taps' weights resident in LDS (k_conv_f16_c32_pool)
static bool take_c32_pool(const F16Conv &q, F16Step &s)
{
    const LayerDesc &l = q.l;
    if (!q.fuse_pool || s.a.Cp_in != 32 || l.size != 3 || l.n != 64 || l.h % 16 || l.w % 16 || s.a.Cp_out < 64 ||
        ((size_t)kLead + (size_t)q.B * s.a.PL) * 64 >= (1ull << 32) || q.o.f16_no_c32)
        return false;
    s.T = q.B * (l.h / 16) * (l.w / 16);
    use(s, FK_C32_POOL); s.store = FS_POOL_ONLY;
    s.grid = dim3((unsigned)std::min(s.T, 512)); s.lds = (9 * 64 + 336) * 64;   // two workgroups per CU, weights staged once each
    return true;
}
// the implicit GEMM on 128-row tiles (32 pool windows where the pool is fused) x bn channels: takes every layer
// (a 256x128 tile with 8 wavefronts and per-tap A staging was measured 8 % SLOWER than 128x128
//  with two workgroups per CU: without the halo reuse the bigger tile only adds barrier cost)
static bool take_gemm(const F16Conv &q, F16Step &s, int bn)
{
    static const F16Kid kid[2][4] = {{FK_GLDS_64_SP, FK_GLDS_64, FK_REG_64_64, FK_REG_64_32}, {FK_GLDS_128_SP, FK_GLDS_128, FK_REG_128_64, FK_REG_128_32}};
    const int m_tiles = s.a.pool ? (s.a.npool + 31) / 32 : (s.a.npix + 127) / 128;
    s.a.n_tiles = round_up(q.l.n, bn) / bn; s.grid = dim3(m_tiles * s.a.n_tiles);
    use(s, kid[bn == 128][q.split ? 0 : (q.glds ? 1 : (q.bk64 ? 2 : 3))]);
    return true;
}
// dense halo tile: 256 pixels + W+1 on either side, rounded to 8-row groups, + 8 zero rows (A: two buffers of lt_rows x 128 B)
static int halo_lt_rows(int w) { return round_up(256 + 2 * (w + 1), 8) + 8; }
// persistent halo-tile kernel: the workgroup walks its tiles, the next tile's staging overlaps this one's tail
static bool take_halo_p(const F16Conv &q, F16Step &s)
{
    static const F16Kid kid[2][3] = {{FK_HALO_P_128_SP, FK_HALO_P_128_M16, FK_HALO_P_128}, {FK_HALO_P_256_SP, FK_HALO_P_256_M16, FK_HALO_P_256}};
    const LayerDesc &l = q.l; ConvF16Args &a = s.a;
    if (!q.glds || l.size != 3 || l.n % kBN || !q.persist_ok || q.fuse_pool) return false;
    const int lt_rows = halo_lt_rows(l.w);
    const size_t a_bytes = (size_t)2 * lt_rows * 128;
    const bool off32 = ((size_t)kLead + (size_t)q.B * a.PL) * std::max(a.Cp_in, a.Cp_out) * 2 < (1ull << 32);
    const bool wide = l.n % 256 == 0 && a_bytes + (size_t)2 * 256 * 128 <= kLdsCap;
    const size_t bn = wide ? 256 : 128, lds = a_bytes + 2 * bn * 128;
    if (!off32 || lds > kLdsCap || lt_rows - 8 > 8 * 8 * 8) return false;
    a.n_tiles = l.n / (int)bn; s.T = ((a.npix + 255) / 256) * a.n_tiles;
    // (Launched with one tile per workgroup - the same kernel, only the LDS-free epilogue and the operand order
    //  differ from k_conv_f16_halo - it measured 2.8 % slower over the pass at batch 256.)
    s.grid = persistent_grid(s.T);
    s.lds = (unsigned)lds; s.lt_rows = lt_rows; s.store = FS_FULL;
    use(s, kid[wide][q.split ? 0 : (q.o.f16_m16 ? 1 : 2)]);
    return true;
}
// 3x3 layers: halo-tile kernel (input tile staged once per 64-channel chunk, nine taps read it
// shifted) wherever its LDS arena fits: 2 x lt_rows x 128 B (A) + NB x BN x 128 B (B) + fo table
static bool take_halo(const F16Conv &q, F16Step &s)
{
    const LayerDesc &l = q.l, &nx = kNet[q.i + 1]; ConvF16Args &a = s.a;
    if (!q.glds || l.size != 3 || l.n % kBN || q.o.f16_no_halo || q.fuse_pool) return false;
    const int lt_rows = halo_lt_rows(l.w);
    const size_t a_bytes = (size_t)2 * lt_rows * 128, fo_bytes = 256 * sizeof(int);
    const size_t lds256 = a_bytes + (size_t)2 * 256 * 128 + fo_bytes, lds128 = a_bytes + (size_t)3 * 128 * 128 + fo_bytes;
    const bool wide = l.n % 256 == 0 && lds256 <= kLdsCap && a_bytes + (size_t)2 * 256 * 128 >= (size_t)256 * 264 * 2 && !q.o.f16_no_wide;
    // (the two-buffer 256x128 form that would fit the 104x104 layers runs one workgroup per CU and measured
    //  6 % slower there than the 128x128 kernel with two: only the shapes below are used)
    if (lt_rows - 8 > 8 * 8 * 8 || a_bytes < (size_t)256 * kCtRow * 2 || !(wide || lds128 <= kLdsCap) || !q.in32) return false;
    s.lt_rows = lt_rows; s.store = FS_FULL;   // (the kernels' dynamic-LDS limit was raised for this device in load_weights_fp32)
    a.n_tiles = wide ? l.n / 256 : l.n / kBN;
    s.grid = dim3(((a.npix + 255) / 256) * a.n_tiles); s.lds = (unsigned)(wide ? lds256 : lds128);   // (without `wide`: the three-buffer 128 form fits)
    // a 256-channel 3x3 whose only consumer is a 1x1 down to 128 channels (layer 8 -> 9): the 1x1 runs in the epilogue
    const bool fuse1 = wide && !q.split && !q.o.f16_no_fuse1x1 && !q.o.f16_m16 && !q.o.f16_w8 && l.n == 256 && a.n_tiles == 1 && nx.type == L_CONV &&
                       nx.size == 1 && nx.c == 256 && nx.n == 128 && nx.leaky == l.leaky && nx.h == l.h && nx.w == l.w && next_is_only_reader(q.i);
    if (fuse1) { fuse_1x1_next(q, s); use(s, FK_HALO_256_1X1); }
    else if (!wide) use(s, q.split ? FK_HALO_128_SP : FK_HALO_128);
    else if (q.split) use(s, FK_HALO_256_SP);
    else if (q.o.f16_m16) use(s, FK_HALO_256_M16);
    else if (!q.o.f16_w8) use(s, FK_HALO_256);   // 16 wavefronts of 64x64 (4 per SIMD, +4 %) instead of 8 of 128x64
    else use(s, FK_HALO_256_W8);
    return true;
}
static int select_f16_table(const Y2Options &o, bool split, int B, F16Table &T)
{
    T = F16Table();
    {   // layers 0+1 fused: conv 3->32 + leaky + 2x2 pool straight from the float frames
        const HalfGeom g = f16_geom(1, split, B);
        F16Step s;
        s.layer = 0; s.B = B; s.t_out = 1; s.oWp = g.Wp; s.oPL = g.PL;   // (booked to layer 0; the pool, layer 1, has no launch of its own)
        if (!o.f16_no_mfma0) {   // 416 = 26 x 16 = 13 x 32: the tile grid is exact.  split: the MFMA form on (hi, lo) pairs: three MFMAs per product, (hi, lo) out: 128-halve items
            use(s, split ? FK_C0_MFMA_SP : FK_C0_MFMA);
            s.T = B * (416 / 16) * (416 / 32);
            // persistent workgroups, Y2_CONV0_WGS per CU; split: 161 registers: three workgroups per CU are resident - a fourth would run behind them
            s.grid = dim3((unsigned)std::min(s.T, 256 * (split ? 3 : Y2_CONV0_WGS)));
        } else {   // (option f16_no_mfma0) split: fp32 VALU form, nothing rounded before the pool
            use(s, split ? FK_C0_VALU_SP : FK_C0_VALU);
            s.grid = dim3(blocks_for((long)B * g.H * g.W, 256), 2);
        }
        T.steps.push_back(s);
        if (!o.f16_no_mfma0) {   // the same tiles, grid and output from image bytes (the images entries)
            const F16Kid kid[Y2_KIND_COUNT][2] = {{FK_C0_U8, FK_C0_U8_SP}, {FK_C0_YUYV, FK_C0_YUYV_SP}, {FK_C0_NV12, FK_C0_NV12_SP}, {FK_C0_I420, FK_C0_I420_SP},
                                                  {FK_C0_BGR24, FK_C0_BGR24_SP}, {FK_C0_RGBA32, FK_C0_RGBA32_SP}, {FK_C0_BGRA32, FK_C0_BGRA32_SP}};
            const F16Kernel &u8 = kF16Kernels[kid[Y2_KIND_BYTES][split ? 1 : 0]];
            T.u8 = s; T.u8.kernel = u8.name; T.launch_u8 = u8.launch_u8;
            for (int kind = 0; kind < Y2_KIND_COUNT; ++kind) {
                const F16Kernel &k = kF16Kernels[kid[kind][split ? 1 : 0]];
                T.pix_kernel[kind] = k.name; T.launch_pix[kind] = k.launch_u8;
            }
        }
    }
    // (a fused pool or 1x1 stores the tensor of the layer it swallowed, so every step reads the tensor the wiring names)
    int skip_pool = -1, fused_conv = -1;
    for (int i = 2; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        const NetWire &w = kWire[i];
        switch (l.type) {
        case L_CONV: {
            if (i == fused_conv) break;   // this 1x1 layer ran inside the launch of the 3x3 before it: its tensor exists already
            F16Step s;
            s.layer = i; s.B = B; s.w_ord = w.ord;
            s.t_in = w.src; s.t_out = w.to_region ? -1 : i;
            ConvF16Args &a = s.a;
            a.B = B; a.H = l.h; a.W = l.w; a.Wp = l.w + 1; a.PL = (l.h + 1) * (l.w + 1); a.npix = B * l.h * l.w;
            a.Cp_in = f16_geom(s.t_in, split, B).Cp; a.Cp_out = f16_geom(i, split, B).Cp;   // (0 for the region buffer)
            a.N = l.n; a.leaky = l.leaky; a.KS = l.size; a.n_tiles = 1; a.stamp = o.stamp_layer == i;
            a.out_ch_off = w.ch_off; a.n_store = w.to_region ? l.n : round_up(l.n, 32);
            a.split_n = split && !w.to_region ? part_stride(w.C) : 0;
            set_fast_div(a);
            s.store = w.to_region ? FS_REGION : FS_FULL_OR_POOL;
            // Conv layers whose only consumer is the 2x2 pool after them (2 and 6; 10 runs the halo kernel, 16 also
            // feeds the route) store the pooled tensor directly: MFMA rows ordered by pool window, max in the epilogue.
            // The persistent halo kernel takes the 104x104 layers EXCEPT layer 6: it stores the full-resolution tensor only
            // (FS_FULL), and the pool kernel that then has to follow (0.08 ms at batch 128) costs more than the conv gains.
            const bool pool_next = kNet[i + 1].type == L_MAX && !o.f16_no_poolfuse;
            const bool persist_ok = !o.f16_no_glds && !o.f16_no_halo && !o.f16_no_persist && ((l.w > 52 && !(i == 6 && pool_next)) || o.f16_persist_all);
            const bool bk64 = a.Cp_in % 64 == 0;
            const F16Conv q = {o, split, B, i, l, bk64, bk64 && !o.f16_no_glds, pool_next, persist_ok, (i == 2 || (i == 6 && !persist_ok)) && pool_next,
                               ((size_t)kLead + (size_t)B * a.PL) * a.Cp_in * 2 < (1ull << 32)};
            if (q.fuse_pool) fuse_pool_into_next(q, s);
            if (split && !bk64) return fail(YOLO2_ERROR, "fp16 plan (split): layer %d has %d-channel items, not a multiple of the 64-channel K-step", i, a.Cp_in);
            (void)(take_rw(q, s) || take_ring(q, s) || take_rwc(q, s) || take_c32_pool(q, s) || (l.n <= 64 && take_gemm(q, s, 64)) || take_halo_p(q, s) ||
                   take_halo(q, s) || take_gemm(q, s, kBN));
            if (s.a.pool) skip_pool = i + 1;        // the pool after this layer ...
            if (s.w2_ord >= 0) fused_conv = i + 1;  // ... or the 1x1 after it ran inside this launch
            const HalfGeom dst = f16_geom(s.t_out, split, B);   // every conv step passes the store check against the tensor it names
            const int rc = f16_store_check(s.kernel, s.store, a.pool, B, a.H, a.W, a.Cp_out, a.out_ch_off, a.n_store, a.oWp, a.oPL, a.npix, a.npool, dst.B,
                                           dst.H, dst.W, dst.Cp, s.store == FS_REGION ? 0 : a.split_n);
            if (rc) return rc;
            T.steps.push_back(s);
            break;
        }
        case L_MAX: {
            if (i == skip_pool) break;   // already produced by the conv before it
            const HalfGeom gi = f16_geom(w.src, split, B), go = f16_geom(i, split, B);
            F16Step s;
            s.layer = i; s.B = B; s.t_in = w.src; s.t_out = i;
            s.oCp = go.Cp; s.OH = go.H; s.OW = go.W; s.iWp = gi.Wp; s.iPL = gi.PL; s.oWp = go.Wp; s.oPL = go.PL;
            if (split) s.oPS = part_stride(go.C);
            use(s, split ? FK_MAXPOOL_SP : FK_MAXPOOL);
            s.grid = dim3(blocks_for((long)B * go.H * go.W * ((split ? s.oPS : go.Cp) / 8), 256));
            T.steps.push_back(s);
            break;
        }
        case L_REORG: {
            const HalfGeom gi = f16_geom(w.src, split, B), go = f16_geom(i, split, B);
            F16Step s;
            s.layer = i; s.B = B; s.t_in = w.src; s.t_out = i;
            s.iCp = gi.Cp; s.iWp = gi.Wp; s.iPL = gi.PL; s.oCp = go.Cp; s.oWp = go.Wp; s.oPL = go.PL;
            if (split) { s.iPS = part_stride(gi.C); s.oPS = part_stride(go.C); }
            use(s, split ? FK_REORG_SP : FK_REORG);
            s.grid = dim3(blocks_for((long)B * (split ? 3 * 128 : 128) * 169, 256));   // one thread per channel pair (and part)
            T.steps.push_back(s);
            break;
        }
        default: break;  // route: concat by placement; region: the last conv already wrote the dense fp32 tensor
        }
    }
    // diagnostic only (f16_skip): drop launches from the table (wrong results), to price them inside the overlapped step
    T.steps.erase(std::remove_if(T.steps.begin(), T.steps.end(), [&](const F16Step &s) {
        const LayerDesc &l = kNet[s.layer]; const int k = o.f16_skip;
        return ((k & 1) && (s.layer == 5 || s.layer == 9)) || ((k & 2) && s.layer == 0) || ((k & 4) && (s.layer == 2 || s.layer == 4 || s.layer == 6)) ||
               ((k & 8) && (l.type == L_MAX || l.type == L_REORG)) || ((k & 16) && l.type == L_CONV && l.size == 1 && s.layer != 5 && s.layer != 9) ||
               ((k & 32) && l.type == L_CONV && l.size == 3 && l.w == 13);
    }), T.steps.end());
    T.batch = B;
    return YOLO2_SUCCESS;
}

// ---- the table as text: one line per step with every field selection sets (yolo2_hip_f16_plan_describe, the `verbose` plan print)
static std::string f16_table_text(const F16Table &T, const char *prefix)
{
    auto tensor = [](int t, const char *none) { return t < 0 ? std::string(none) : (kWire[t].cat >= 0 ? std::string("cat") : "t" + std::to_string(t)); };
    std::string out;
    char buf[960], args[320];
    for (const F16Step &s : T.steps) {
        const ConvF16Args &a = s.a;
        snprintf(args, sizeof(args), "-");
        if (s.w_ord >= 0)   // a conv step: the ConvF16Args scalars in declaration order
            snprintf(args, sizeof(args), "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%u,%u,%u,%u,%d,%d", a.B, a.H, a.W, a.Wp, a.PL, a.Cp_in, a.Cp_out, a.N,
                     a.out_ch_off, a.n_store, a.npix, a.leaky, a.KS, a.n_tiles, a.pool, a.oWp, a.oPL, a.npool, a.mHW, a.sHW, a.mW, a.sW, a.stamp, a.split_n);
        snprintf(buf, sizeof(buf), "%sL%d %s store=%d grid=%u,%u block=%u lds=%u lt_rows=%d T=%d B=%d in=%s out=%s w=%d w2=%d a=%s pr=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n",
                 prefix, s.layer, s.kernel, (int)s.store, s.grid.x, s.grid.y, s.block.x, s.lds, s.lt_rows, s.T, s.B, tensor(s.t_in, s.layer == 0 ? "frames" : "-").c_str(),
                 tensor(s.t_out, s.store == FS_REGION ? "region" : "-").c_str(), s.w_ord, s.w2_ord, args, s.iCp, s.iWp, s.iPL, s.oCp, s.oWp, s.oPL, s.OH, s.OW, s.iPS, s.oPS);
        out += buf;
    }
    if (T.launch_u8) out += std::string(prefix) + "u8 " + T.u8.kernel + "\n" + prefix + "yuyv " + T.pix_kernel[Y2_KIND_YUYV] + "\n";   // (the text of the recorded tables)
    return out;
}

// Test hook (no GPU needed): the table selection makes for (options, split, batch), as the text above.
extern "C" int yolo2_hip_f16_plan_describe(const char *options, int split, int batch, char *buf, int cap)
{
    if (split != 0 && split != 1) return fail(YOLO2_ERROR, "split must be 0 (fp16) or 1 (fp32 tolerance), not %d", split);
    if (batch <= 0 || batch > 4096) return fail(YOLO2_ERROR, "batch %d out of range", batch);
    Y2Options o;
    const std::string opts = options ? options : "";
    for (size_t p = opts.find_first_not_of(' '); p != std::string::npos;) {
        const size_t e = std::min(opts.find(' ', p), opts.size()), eq = opts.find('=', p);
        if (eq >= e || o.set(opts.substr(p, eq - p).c_str(), opts.substr(eq + 1, e - eq - 1).c_str()) != 0)
            return fail(YOLO2_ERROR, "unknown option or value out of range: %s", opts.substr(p, e - p).c_str());
        p = opts.find_first_not_of(' ', e);
    }
    F16Table T;
    if (const int rc = select_f16_table(o, split != 0, batch, T)) return rc;
    const std::string text = f16_table_text(T, "");
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", text.c_str());
    return (int)text.size();
}

// ---- binding: the addresses of one step, from the context's tensors (ensure_f16_batch) and weight offsets
static int bind_f16_step(const yolo2_hip_ctx *c, F16Step &s)
{
    if ((s.t_in >= 0 && !c->h_out[s.t_in].d) || (s.t_out >= 0 && !c->h_out[s.t_out].d)) return fail(YOLO2_ERROR, "fp16 plan: layer %d names a tensor that is not allocated", s.layer);
    if (s.t_in >= 0) s.in = c->h_out[s.t_in].d;
    if (s.t_out >= 0) s.out = c->h_out[s.t_out].d;
    if (s.layer == 0) { s.w0 = c->w0f; s.bias = c->w0f + 27 * 32; }
    if (s.w_ord >= 0) { s.w = c->wh + c->wh_off[s.w_ord]; s.bias = c->biasf + c->biasf_off[s.w_ord]; }
    if (s.w2_ord >= 0) { s.w2 = c->wh + c->wh_off[s.w2_ord]; s.bias2 = c->biasf + c->biasf_off[s.w2_ord]; }
    return YOLO2_SUCCESS;
}

// Builds the table for batch B: selection, then binding to the context's tensors (they exist: ensure_f16_batch).
static int build_f16_plan(yolo2_hip_ctx *c, int B)
{
    F16Plan &P = *c->f16_plan;
    int rc = select_f16_table(P.opt, c->split, B, P);
    for (F16Step &s : P.steps) if (!rc) rc = bind_f16_step(c, s);
    if (!rc && P.launch_u8) rc = bind_f16_step(c, P.u8);
    if (rc) { P.batch = 0; P.steps.clear(); return rc; }
    if (P.opt.verbose) fputs(f16_table_text(P, "[yolo2_hip] fp16 plan ").c_str(), stderr);   // (plan construction, not the launch path)
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
    c->f16_plan->lanes = lanes;
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
        if (ok) l->f16_plan->opt = c->f16_plan->opt;   // a lane runs the parent's kernel selection
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
// for a chunk of YUYV / NV12 / I420 frames (kind: Y2PixKind), the step from those.
static int run_f16(yolo2_hip_ctx *c, uint64_t frames_dev, const uint8_t *lb, int lb_first, int kind, int batch, uint64_t region_dev,
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
    const int want_lanes = c->f16_plan->lanes;
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
            const int rc = run_f16(l, lb ? 0 : frames_dev + (uint64_t)i * half * YOLO2_FRAME_ELEMS * sizeof(float), lb, lb_first + i * half, kind, half,
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
    const F16LaunchU8 from_bytes = P.launch_pix[kind];
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
    return run_f16(c, frames_dev, nullptr, 0, Y2_KIND_BYTES, batch, region_dev, stream);
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
    if (kWire[layer_idx].to_region) return fail(YOLO2_ERROR, "layer %d's output is the region tensor the run returns", layer_idx);
    const LayerDesc &l = kNet[layer_idx];
    if (l.type == L_ROUTE) return fail(YOLO2_ERROR, "route layer %d has no tensor of its own", layer_idx);
    if (!c->f16_plan || c->f16_plan->batch != c->f16_last_batch) return fail(YOLO2_ERROR, "no launch table for the last run");
    const bool cat = kWire[layer_idx].cat >= 0;
    const yolo2_hip_ctx::HalfTensor &t = c->h_out[layer_idx];
    bool written = false;   // from the table itself: some step stores into this tensor (a member of the concat: the step of that layer)
    for (const F16Step &s : c->f16_plan->steps)
        if (t.d && s.out == t.d && (!cat || s.layer == layer_idx)) written = true;
    if (!written)
        return fail(YOLO2_ERROR, "layer %d's tensor is not written by the current fp16 plan (its launch is fused or it has none)", layer_idx);
    const int C = l.type == L_MAX ? l.c : (l.type == L_REORG ? 4 * l.c : l.n);
    const int ps = c->split ? part_stride(kWire[layer_idx].C) : t.Cp;
    const int g[8] = {C, t.Cp, t.H, t.W, t.Wp, which == 0 ? t.PL : (which == 1 ? kLead : kTail), ps, kWire[layer_idx].ch_off};
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

bool y2_f16_images_fused(const yolo2_hip_ctx *run) { return !run->f16_plan->opt.f16_no_mfma0; }

int y2_f16_run_images(yolo2_hip_ctx *run, const uint8_t *lb, int kind, int batch, float *region_dev, hipStream_t st)
{
    if (!lb) return fail(YOLO2_ERROR, "null buffer address");
    return run_f16(run, 0, lb, 0, kind, batch, (uint64_t)(uintptr_t)region_dev, st);
}

const char *y2_f16_images_kernel(const yolo2_hip_ctx *run, int kind)
{
    if (!run->f16_lanes.empty() && run->f16_last_laned) run = run->f16_lanes[0];
    if (!run->f16_plan || !run->f16_plan->launch_u8) return "";
    return run->f16_plan->pix_kernel[kind];
}
