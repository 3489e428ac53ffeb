// yolo2_hip.hip -- the part of libyolo2_hip.so (include/yolo2_hip.h) every tier shares: error slot, model tables, context
// lifecycle, HBM helpers, per-layer profiling, GPU pre-processing and the host-buffer streaming entries.  The tiers themselves:
// yolo2_driver.hip (reference driver interface), yolo2_int16.hip, yolo2_fp16.hip, yolo2_fp32.hip (y2_internal.hpp has the map).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "y2_internal.hpp"
#include "kernels_pre.hpp"
#include "kernels_pix.hpp"   // after kernels_pre.hpp: uses its structs

using namespace y2;

// ---------------------------------------------------------------------------- errors

static thread_local char g_err[512] = "";
static const bool g_verbose = y2_process_options().verbose;   // latched once: no getenv on any launch path

int y2_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    if (g_verbose) fprintf(stderr, "[yolo2_hip] %s\n", g_err);
    return code;
}

extern "C" const char *yolo2_hip_last_error(void) { return g_err; }
// for the library's other translation units (yolo2_multi.hip, yolo2_post.hip): same thread-local message slot
extern "C" int yolo2_hip_set_error(int code, const char *msg) { return fail(code, "%s", msg ? msg : ""); }

// ---------------------------------------------------------------------------- model tables
// Host data.  The wiring is computed from them at compile time, so they are constexpr - in the host pass only: HIP puts a constexpr
// global into the device code object as well, where no kernel wants them.
#ifdef __HIP_DEVICE_COMPILE__
#define Y2_HOST_TABLE const
#else
#define Y2_HOST_TABLE constexpr
#endif

extern "C" Y2_HOST_TABLE int yolo2_weight_len[YOLO2_N_CONV] = {864, 18432, 73728, 8192, 73728, 294912, 32768, 294912,
                                                               1179648, 131072, 1179648, 131072, 1179648, 4718592,
                                                               524288, 4718592, 524288, 4718592, 9437184, 9437184,
                                                               32768, 11796480, 435200};
extern "C" Y2_HOST_TABLE int yolo2_bias_len[YOLO2_N_CONV] = {32, 64, 128, 64, 128, 256, 128, 256, 512, 256, 512, 256,
                                                             512, 1024, 512, 1024, 512, 1024, 1024, 1024, 64, 1024, 425};

extern "C" long yolo2_strip_int16_layer_pad(const int16_t *file, size_t file_elems, const int *layer_len,
                                            int n_layers, int16_t *dst)
{
    size_t fo = 0, oo = 0;
    for (int l = 0; l < n_layers; ++l) {
        const size_t len = (size_t)layer_len[l];
        if (fo + len > file_elems) return -1;
        memcpy(dst + oo, file + fo, len * sizeof(int16_t));
        fo += len + (len & 1);  // yolo2_model.cpp:215-220
        oo += len;
    }
    return (long)oo;
}

// config/yolov2.cfg as parsed by the reference; the C host re-derives the same
// table from the .cfg file and checks it against this one before using the batched entry.
Y2_HOST_TABLE LayerDesc kNet[32] = {
    {L_CONV, 3, 416, 416, 32, 3, 1},    {L_MAX, 32, 416, 416, 32, 2, 0},   {L_CONV, 32, 208, 208, 64, 3, 1},
    {L_MAX, 64, 208, 208, 64, 2, 0},    {L_CONV, 64, 104, 104, 128, 3, 1}, {L_CONV, 128, 104, 104, 64, 1, 1},
    {L_CONV, 64, 104, 104, 128, 3, 1},  {L_MAX, 128, 104, 104, 128, 2, 0}, {L_CONV, 128, 52, 52, 256, 3, 1},
    {L_CONV, 256, 52, 52, 128, 1, 1},   {L_CONV, 128, 52, 52, 256, 3, 1},  {L_MAX, 256, 52, 52, 256, 2, 0},
    {L_CONV, 256, 26, 26, 512, 3, 1},   {L_CONV, 512, 26, 26, 256, 1, 1},  {L_CONV, 256, 26, 26, 512, 3, 1},
    {L_CONV, 512, 26, 26, 256, 1, 1},   {L_CONV, 256, 26, 26, 512, 3, 1},  {L_MAX, 512, 26, 26, 512, 2, 0},
    {L_CONV, 512, 13, 13, 1024, 3, 1},  {L_CONV, 1024, 13, 13, 512, 1, 1}, {L_CONV, 512, 13, 13, 1024, 3, 1},
    {L_CONV, 1024, 13, 13, 512, 1, 1},  {L_CONV, 512, 13, 13, 1024, 3, 1}, {L_CONV, 1024, 13, 13, 1024, 3, 1},
    {L_CONV, 1024, 13, 13, 1024, 3, 1}, {L_ROUTE, 0, 0, 0, 0, 0, 0},       {L_CONV, 512, 26, 26, 64, 1, 1},
    {L_REORG, 64, 26, 26, 256, 0, 0},   {L_ROUTE, 0, 0, 0, 0, 0, 0},       {L_CONV, 1280, 13, 13, 1024, 3, 1},
    {L_CONV, 1024, 13, 13, 425, 1, 0},  {L_REGION, 425, 13, 13, 0, 0, 0},
};

// The wiring (y2_internal.hpp): kNet plus the cfg's two [route] lines, layers=-9 at layer 25 and layers=-1,-4 at layer 28.
#ifndef __HIP_DEVICE_COMPILE__
struct RouteDef { int layer, n, src[4]; };
constexpr RouteDef kRoutes[] = {{25, 1, {16}}, {28, 2, {27, 24}}};

constexpr NetWiring make_wiring()
{
    NetWiring t = {};
    int ord = 0, own_c[32] = {};
    long w_off = 0, b_off = 0;
    for (int i = 0; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        NetWire &w = t.layer[i];
        w.ord = -1; w.cat = -1; w.reader = -1;
        w.src = i == 0 ? -1 : (kNet[i - 1].type == L_ROUTE ? t.layer[i - 1].src : i - 1);
        switch (l.type) {
        case L_CONV:
            w.ord = ord; w.w_off = w_off; w.b_off = b_off;
            t.conv_layer[ord] = i;
            w_off += yolo2_weight_len[ord]; b_off += yolo2_bias_len[ord]; ord++;
            w.C = l.n; w.H = l.h; w.W = l.w;
            break;
        case L_MAX: w.C = l.c; w.H = l.h / 2; w.W = l.w / 2; break;
        case L_REORG: w.C = l.n; w.H = l.h / 2; w.W = l.w / 2; break;
        case L_REGION: w.C = l.c; w.H = l.h; w.W = l.w; break;
        case L_ROUTE:
            for (const RouteDef &r : kRoutes) {
                if (r.layer != i) continue;
                w.n_route = r.n;
                for (int k = 0; k < r.n; ++k) w.route[k] = r.src[k];
            }
            if (w.n_route == 1) {            // an alias of its source
                w.src = kNet[w.route[0]].type == L_ROUTE ? t.layer[w.route[0]].src : w.route[0];
                w.C = t.layer[w.src].C; w.H = t.layer[w.src].H; w.W = t.layer[w.src].W;
            } else {                         // the concat tensor: its members in the cfg's order
                w.src = w.cat = i;
                w.H = t.layer[w.route[0]].H; w.W = t.layer[w.route[0]].W;
                for (int k = 0; k < w.n_route; ++k) {
                    NetWire &m = t.layer[w.route[k]];
                    m.cat = i; m.ch_off = w.C;
                    w.C += own_c[w.route[k]];
                    if (m.H != w.H || m.W != w.W) w.C = -1;   // (fails the check below)
                    if (kNet[w.route[k]].type == L_CONV) t.cat_conv = w.route[k];
                    if (kNet[w.route[k]].type == L_REORG) t.cat_feed = m.src;
                }
                for (int k = 0; k < w.n_route; ++k) t.layer[w.route[k]].C = w.C;
            }
            break;
        }
        own_c[i] = w.C;
    }
    for (int i = 0; i < 32; ++i) {           // who reads what: a reader of the concat tensor reads every member
        const int s = t.layer[i].src;
        if (kNet[i].type == L_ROUTE || s < 0) continue;
        for (int j = 0; j <= s; ++j)
            if (j == s || t.layer[j].cat == s) {
                if (t.layer[j].readers++ == 0) t.layer[j].reader = i;
                t.layer[j].to_region |= kNet[i].type == L_REGION;
            }
    }
    return t;
}
// every layer's c, h, w are the shape of the tensor it reads (the concat's channel sum included), and the streams add up
constexpr bool wiring_ok(const NetWiring &t)
{
    for (int i = 0; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        const int s = t.layer[i].src;
        if (l.type == L_ROUTE) continue;
        if (s < 0 ? (l.c != 3 || i != 0) : (t.layer[s].C != l.c || t.layer[s].H != l.h || t.layer[s].W != l.w)) return false;
        if (l.type == L_CONV && (yolo2_weight_len[t.layer[i].ord] != l.c * l.n * l.size * l.size || yolo2_bias_len[t.layer[i].ord] != l.n)) return false;
    }
    const NetWire &last = t.layer[t.conv_layer[YOLO2_N_CONV - 1]];
    return last.w_off + yolo2_weight_len[YOLO2_N_CONV - 1] == YOLO2_N_WEIGHTS && last.b_off + yolo2_bias_len[YOLO2_N_CONV - 1] == YOLO2_N_BIAS;
}
constexpr NetWiring kWiring = make_wiring();
static_assert(wiring_ok(kWiring), "kNet, the route lists and the stream lengths do not describe one network");
#endif

extern "C" int yolo2_hip_layer_routes(int i, int src[4])
{
    if (i < 0 || i >= 32 || !src) return YOLO2_ERROR;
    for (int k = 0; k < kWire[i].n_route; ++k) src[k] = kWire[i].route[k];
    return kWire[i].n_route;
}
// Test hook: the wiring of layer i as {ord, w_off, b_off, src, cat, ch_off, readers, reader, to_region, C, H, W}
extern "C" int yolo2_hip_debug_layer_wiring(int i, int out[12])
{
    if (i < 0 || i >= 32 || !out) return YOLO2_ERROR;
    const NetWire &w = kWire[i];
    const int v[12] = {w.ord, (int)w.w_off, (int)w.b_off, w.src, w.cat, w.ch_off, w.readers, w.reader, w.to_region ? 1 : 0, w.C, w.H, w.W};
    for (int k = 0; k < 12; ++k) out[k] = v[k];
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_num_layers(void) { return 32; }
extern "C" int yolo2_hip_layer_desc(int i, int desc[9])
{
    if (i < 0 || i >= 32 || !desc) return YOLO2_ERROR;
    const LayerDesc &l = kNet[i];
    static const int type_code[] = {0, 1, 3, 2, 4};  // yolo2_config.h:118-122 numbering
    const int stride = l.type == L_MAX || l.type == L_REORG ? 2 : (l.type == L_CONV ? 1 : 0);
    const int pad = l.type == L_CONV && l.size == 3 ? 1 : 0;
    const int v[9] = {type_code[l.type], l.c, l.h, l.w, l.n, l.size, stride, pad, l.leaky};
    for (int k = 0; k < 9; ++k) desc[k] = v[k];
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- HBM helpers

std::atomic<size_t> y2_live_bytes[2];

extern "C" int yolo2_hip_debug_live_bytes(size_t *device_bytes, size_t *pinned_bytes)
{
    if (!device_bytes || !pinned_bytes) return fail(YOLO2_ERROR, "null argument");
    *device_bytes = y2_live_bytes[0];
    *pinned_bytes = y2_live_bytes[1];
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_alloc(size_t bytes, uint64_t *dev_addr)
{
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes), YOLO2_MMAP_ERROR);
    *dev_addr = (uint64_t)(uintptr_t)p;
    return YOLO2_SUCCESS;
}
extern "C" int yolo2_hip_alloc_on(yolo2_hip_ctx *c, size_t bytes, uint64_t *dev_addr)
{
    if (!c || !dev_addr) return fail(YOLO2_ERROR, "null argument");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    return yolo2_hip_alloc(bytes, dev_addr);
}
extern "C" void yolo2_hip_free(uint64_t dev_addr) { (void)hipFree((void *)(uintptr_t)dev_addr); }
extern "C" int yolo2_hip_memcpy_h2d(uint64_t dst, const void *src, size_t bytes)
{
    HIP_TRY(hipMemcpy((void *)(uintptr_t)dst, src, bytes, hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}
extern "C" int yolo2_hip_memcpy_d2h(void *dst, uint64_t src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, (const void *)(uintptr_t)src, bytes, hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}
extern "C" int yolo2_hip_memset(uint64_t dst, int value, size_t bytes)
{
    HIP_TRY(hipMemset((void *)(uintptr_t)dst, value, bytes), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- context lifecycle

extern "C" int yolo2_hip_create(int device, yolo2_hip_ctx **out)
{
    if (!out) return fail(YOLO2_ERROR, "null ctx pointer");
    if (device < 0 || device >= yolo2_hip_device_count())
        return fail(YOLO2_INIT_ERROR, "no HIP device %d (the GPU path has no CPU fallback)", device);
    HIP_TRY(hipSetDevice(device), YOLO2_INIT_ERROR);
    yolo2_hip_ctx *c = new (std::nothrow) yolo2_hip_ctx();
    if (!c) return fail(YOLO2_ERROR, "out of host memory");
    c->device = device;
    c->opt = Y2Options::from_env();   // the ONLY read of the YOLO2_* switches for this context (yolo2_hip_set_option changes them later)
    *out = c;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_ctx_device(yolo2_hip_ctx *c) { return c ? c->device : -1; }

void y2_free_activations(yolo2_hip_ctx *c)
{
    c->ks_trip_own.reset();
    c->ks_trip = nullptr;
    c->ks_trip_bytes = 0;
    y2_free_tensors(c->t_in, c->t_out, c->t_cat, c->batch);
}

void y2_destroy_lanes(yolo2_hip_ctx *c)
{
    c->lane_first.clear();
    for (yolo2_hip_ctx *l : c->lanes) yolo2_hip_destroy(l);
    c->lanes.clear();
    c->laned = false;
}

static void pipe_free(PipeBufs &p)
{
    for (int k = 0; k < 2; ++k) {
        if (p.e_in[k]) (void)hipEventDestroy(p.e_in[k]);
        if (p.e_run[k]) (void)hipEventDestroy(p.e_run[k]);
        if (p.e_out[k]) (void)hipEventDestroy(p.e_out[k]);
        for (hipEvent_t &e : p.e_lane[k]) if (e) (void)hipEventDestroy(e);
    }
    if (p.s_in) (void)hipStreamDestroy(p.s_in);
    if (p.s_run) (void)hipStreamDestroy(p.s_run);
    if (p.s_out) (void)hipStreamDestroy(p.s_out);
    p = PipeBufs();   // (its owners free the buffers)
}

// need_hout: the pinned mirror of the region tensor (the entries that return region tensors; the images -> detections entry
// downloads records instead and skips these 2 x 9 MB of pinned memory, which cost ~10 ms each to allocate)
int y2_pipe_ensure(PipeBufs &p, size_t host_in, size_t dev_in, int batch, bool need_hout = true)
{
    if (p.s_in && p.host_in >= host_in && p.dev_in >= dev_in && p.batch >= batch && (!need_hout || p.hout[0])) return YOLO2_SUCCESS;
    need_hout = need_hout || p.hout[0];
    host_in = std::max(host_in, p.host_in);
    dev_in = std::max(dev_in, p.dev_in);
    batch = std::max(batch, p.batch);
    pipe_free(p);
    const size_t felems = (size_t)batch * YOLO2_FRAME_ELEMS, relems = (size_t)batch * YOLO2_REGION_ELEMS;
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k) {
        ok = p.hin[k].alloc(host_in) == YOLO2_SUCCESS && (!need_hout || p.hout[k].alloc(relems) == YOLO2_SUCCESS) &&
             p.dbytes[k].alloc(dev_in) == YOLO2_SUCCESS && p.din[k].alloc(felems) == YOLO2_SUCCESS && p.dout[k].alloc(relems) == YOLO2_SUCCESS &&
             hipEventCreateWithFlags(&p.e_in[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&p.e_run[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&p.e_out[k], hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && hipStreamCreateWithFlags(&p.s_in, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&p.s_run, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&p.s_out, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        pipe_free(p);
        return fail(YOLO2_MMAP_ERROR, "staging buffers for %d frames (+%zu bytes) could not be allocated", batch, host_in);
    }
    p.host_in = host_in; p.dev_in = dev_in; p.batch = batch;
    return YOLO2_SUCCESS;
}

static const bool g_lane_prio = y2_process_options().lane_priority != 0;   // process-wide (the priority pools are): latched once

bool y2_lane0_own_stream() { return g_lane_prio; }

int y2_lane_stream_create(hipStream_t *s)
{
    if (!g_lane_prio) {
        HIP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking), YOLO2_ERROR);
        return YOLO2_SUCCESS;
    }
    int least = 0, greatest = 0;   // numerically lower = higher priority
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least &&
        hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest) == hipSuccess)
        return YOLO2_SUCCESS;
    (void)hipGetLastError();       // a runtime without stream priorities: an ordinary stream (correct, possibly sharing a hardware queue)
    HIP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

extern "C" void yolo2_hip_destroy(yolo2_hip_ctx *c)
{
    if (!c) return;
    yolo2_hip_rccl_finalize(c);   // leaves its communicator, if it joined one (no-op otherwise; never loads librccl)
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    pipe_free(c->pipe);
    y2_anno_free(c);
    y2_anno_jpeg_free(c);
    y2_loop_free(c);
    y2_f16_plan_free(c);
    y2_i8_free(c);
    y2_destroy_lanes(c);
    y2_free_activations(c);
    if (c->lane_stream) (void)hipStreamDestroy(c->lane_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (yolo2_hip_ctx *l : c->f16_lanes) yolo2_hip_destroy(l);
    c->f16_lanes.clear();
    if (c->tol) yolo2_hip_destroy(c->tol);
    c->tol = nullptr;
    if (c->ev_made)
        for (auto &slot : c->ev)
            for (auto &e : slot) (void)hipEventDestroy(e);
    delete c;   // the owners free what this context allocated; what it borrowed (a lane's, the twin's views) stays with the parent
}

// ---------------------------------------------------------------------------- lanes / profiling accessors

extern "C" int yolo2_hip_num_lanes(yolo2_hip_ctx *c) { return c && c->laned ? (int)c->lanes.size() : 1; }
extern "C" int yolo2_hip_num_lanes_fp16(yolo2_hip_ctx *c) { return c && !c->f16_lanes.empty() ? (int)c->f16_lanes.size() : 1; }

int y2_ensure_prof_events(yolo2_hip_ctx *c)
{
    if (c->ev_made) return YOLO2_SUCCESS;
    for (auto &slot : c->ev)
        for (auto &e : slot) HIP_TRY(hipEventCreate(&e), YOLO2_ERROR);
    c->ev_made = true;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_set_profiling(yolo2_hip_ctx *c, int enable)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if (c->laned) {   // with lanes the events of lane 0 are reported (its launches overlap lane 1's)
        c->prof = enable != 0;
        c->prof_runs = 0;
        return yolo2_hip_set_profiling(c->lanes[0], enable);
    }
    if (enable) {
        const int rc = y2_ensure_prof_events(c);
        if (rc) return rc;
    }
    c->prof = enable != 0;
    c->prof_runs = 0;  // (re)start the averaging window
    if (c->tol) (void)yolo2_hip_set_profiling(c->tol, enable);                              // the split-mode twin follows its parent
    if (!c->f16_lanes.empty()) return yolo2_hip_set_profiling(c->f16_lanes[0], enable);   // fp16 lanes: lane 0 is reported
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_layer_times_ms(yolo2_hip_ctx *c, float *ms32)
{
    if (!c || !ms32) return fail(YOLO2_ERROR, "null argument");
    if (c->laned) return yolo2_hip_layer_times_ms(c->lanes[0], ms32);
    if (c->prof_runs == 0 && !c->f16_lanes.empty() && c->f16_lanes[0]->prof_runs > 0) return yolo2_hip_layer_times_ms(c->f16_lanes[0], ms32);
    if (c->prof_runs == 0 && c->tol) return yolo2_hip_layer_times_ms(c->tol, ms32);   // only the split-mode twin has run since profiling was switched on
    if (c->prof_runs == 0 && !c->f16_lanes.empty()) return yolo2_hip_layer_times_ms(c->f16_lanes[0], ms32);
    if (c->prof_runs == 0) return fail(YOLO2_ERROR, "no profiled run yet");
    const int n = (int)std::min<long>(c->prof_runs, yolo2_hip_ctx::kProfSlots);
    for (int i = 0; i < 32; ++i) ms32[i] = 0.f;
    for (int sidx = 0; sidx < n; ++sidx) {
        HIP_TRY(hipEventSynchronize(c->ev[sidx][32]), YOLO2_ERROR);
        for (int i = 0; i < 32; ++i) {
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, c->ev[sidx][i], c->ev[sidx][i + 1]), YOLO2_ERROR);
            ms32[i] += t / n;
        }
    }
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- pre-processing

// The pixel formats (y2_internal.hpp has the fields).  The first two are the u8 entries' channel counts.
static const Y2PixDesc kPixDescs[] = {
    {YOLO2_PIX_GREY8, "GREY8", 1, Y2_KIND_BYTES, 8, false, false, 1},
    {YOLO2_PIX_RGB24, "RGB24", 3, Y2_KIND_BYTES, 24, false, false, 1},
    {YOLO2_PIX_YUYV, "YUYV", 2, Y2_KIND_YUYV, 16, true, false, 4},            // (LbYuyv loads pixel pairs as dwords)
    {YOLO2_PIX_NV12, "NV12", y2::kLbChNv12, Y2_KIND_NV12, 12, true, true, 1},   // (LbYuv420 loads bytes)
    {YOLO2_PIX_I420, "I420", y2::kLbChI420, Y2_KIND_I420, 12, true, true, 1},
    {YOLO2_PIX_BGR24, "BGR24", y2::kLbChBgr24, Y2_KIND_BGR24, 24, false, false, 1},       // (LbPacked<3, .> loads bytes)
    {YOLO2_PIX_RGBA32, "RGBA32", y2::kLbChRgba32, Y2_KIND_RGBA32, 32, false, false, 4},   // (LbPacked<4, .> loads a pixel as one dword)
    {YOLO2_PIX_BGRA32, "BGRA32", y2::kLbChBgra32, Y2_KIND_BGRA32, 32, false, false, 4},
};

const Y2PixDesc *y2_pix_desc(int pixfmt, const char *who)
{
    for (const Y2PixDesc &d : kPixDescs)
        if (d.pixfmt == pixfmt) return &d;
    (void)fail(YOLO2_ERROR, "%s%sunknown pixel format 0x%x (YOLO2_PIX_GREY8, YOLO2_PIX_RGB24, YOLO2_PIX_YUYV, YOLO2_PIX_NV12, YOLO2_PIX_I420, "
                            "YOLO2_PIX_BGR24, YOLO2_PIX_RGBA32 or YOLO2_PIX_BGRA32)",
               who ? who : "", who ? ": " : "", (unsigned)pixfmt);
    return nullptr;
}

const Y2PixDesc *y2_pix_desc_ch(int ch)
{
    for (const Y2PixDesc &d : kPixDescs)
        if (d.ch == ch) return &d;
    return nullptr;
}

int y2_pix_check_parity(const Y2PixDesc &d, int w, int h, const char *who, int frame)
{
    const bool bad_w = d.even_w && (w & 1);
    if (!bad_w && !(d.even_h && (h & 1))) return YOLO2_SUCCESS;
    if (frame < 0) return fail(YOLO2_ERROR, "%s: %s frames have an even %s, not %d", who, d.name, bad_w ? "width" : "height", bad_w ? w : h);
    return fail(YOLO2_ERROR, "%s: %s frames have an even %s, not %d (frame %d)", who, d.name, bad_w ? "width" : "height", bad_w ? w : h, frame);
}

int y2_letterbox_args(int w, int h, int channels, int net_w, int net_h, LetterboxArgs &a, bool pix = false)
{
    const Y2PixDesc *d = y2_pix_desc_ch(channels);
    if (w <= 0 || h <= 0 || net_w <= 1 || net_h <= 1 || !d || (d->kind != Y2_KIND_BYTES && !pix))
        return fail(YOLO2_ERROR, "letterbox: bad image geometry %dx%dx%d -> %dx%d", w, h, channels, net_w, net_h);
    if (const int rc = y2_pix_check_parity(*d, w, h, "letterbox", -1)) return rc;
    if ((long)w * h > (1L << 28)) return fail(YOLO2_ERROR, "letterbox: image too large");
    a.w = w; a.h = h; a.ch = channels; a.net_w = net_w; a.net_h = net_h;
    // letterbox_image, src/core/yolo_image.cpp:148-165
    if (((float)net_w / w) < ((float)net_h / h)) { a.new_w = net_w; a.new_h = (h * net_w) / w; }
    else { a.new_h = net_h; a.new_w = (w * net_h) / h; }
    if (a.new_w < 1 || a.new_h < 1) return fail(YOLO2_ERROR, "letterbox: image aspect too extreme (%dx%d)", w, h);
    a.off_x = (net_w - a.new_w) / 2;
    a.off_y = (net_h - a.new_h) / 2;
    // resize_image, src/core/yolo_image.cpp:89-90 (a one-pixel-wide target divides by zero there too;
    // the value is then never used because its only column takes the c == w-1 branch)
    a.w_scale = (float)(w - 1) / (a.new_w - 1);
    a.h_scale = (float)(h - 1) / (a.new_h - 1);
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_letterbox_u8(uint64_t image_dev, int w, int h, int channels, uint64_t frame_dev, int net_w,
                                      int net_h, void *stream)
{
    if (!image_dev || !frame_dev) return fail(YOLO2_ERROR, "null buffer address");
    LetterboxArgs a;
    int rc = y2_letterbox_args(w, h, channels, net_w, net_h, a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_letterbox_u8, dim3(blocks_for((long)3 * net_w * net_h, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)(uintptr_t)image_dev, (float *)(uintptr_t)frame_dev, a);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// pixfmt -> LetterboxArgs::ch for the _pix entries; 0 and an error for anything else
static int pix_ch(int pixfmt)
{
    const Y2PixDesc *d = y2_pix_desc(pixfmt, nullptr);
    return d ? d->ch : 0;
}

extern "C" int yolo2_hip_letterbox_pix(uint64_t image_dev, int w, int h, int pixfmt, uint64_t frame_dev, int net_w, int net_h,
                                       void *stream)
{
    const Y2PixDesc *d = y2_pix_desc(pixfmt, nullptr);
    if (!d) return YOLO2_ERROR;
    if (d->kind == Y2_KIND_BYTES) return yolo2_hip_letterbox_u8(image_dev, w, h, d->ch, frame_dev, net_w, net_h, stream);
    if (!image_dev || !frame_dev) return fail(YOLO2_ERROR, "null buffer address");
    if (image_dev & (d->align - 1)) return fail(YOLO2_ERROR, "letterbox: a %s frame starts on a %u-byte boundary", d->name, d->align);
    LetterboxArgs a;
    int rc = y2_letterbox_args(w, h, d->ch, net_w, net_h, a, true);
    if (rc) return rc;
    static constexpr decltype(&k_letterbox_yuyv) kernels[Y2_KIND_COUNT] = {nullptr,           k_letterbox_yuyv,   k_letterbox_nv12,  k_letterbox_i420,
                                                                           k_letterbox_bgr24, k_letterbox_rgba32, k_letterbox_bgra32};
    const auto kernel = kernels[d->kind];
    hipLaunchKernelGGL(kernel, dim3(blocks_for((long)3 * net_w * net_h, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)(uintptr_t)image_dev, (float *)(uintptr_t)frame_dev, a);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// the chunk letterbox of every kind of staging buffer (Y2PixKind: what the table items' frames are), and its name
const char *y2_letterbox_batch_kernel(int kind)
{
    static const char *const names[Y2_KIND_COUNT] = {"k_letterbox_u8_batch",    "k_letterbox_yuyv_batch",   "k_letterbox_nv12_batch",  "k_letterbox_i420_batch",
                                                     "k_letterbox_bgr24_batch", "k_letterbox_rgba32_batch", "k_letterbox_bgra32_batch"};
    return names[kind];
}

void y2_launch_letterbox_batch(int kind, const uint8_t *dbytes, float *din, int batch, hipStream_t st)
{
    const dim3 grid(blocks_for((long)YOLO2_FRAME_ELEMS, 256), batch);
    static constexpr decltype(&k_letterbox_u8_batch) kernels[Y2_KIND_COUNT] = {k_letterbox_u8_batch,    k_letterbox_yuyv_batch,   k_letterbox_nv12_batch,
                                                                               k_letterbox_i420_batch,  k_letterbox_bgr24_batch,  k_letterbox_rgba32_batch,
                                                                               k_letterbox_bgra32_batch};
    hipLaunchKernelGGL(kernels[kind], grid, dim3(256), 0, st, dbytes, din, (int)YOLO2_FRAME_ELEMS);   // the whole chunk in one launch
}

// Camera-style entry: n images of arbitrary sizes as host bytes -> region tensors, in chunks of
// `batch` images.  The bytes (not the 4x larger float frames) cross PCIe; letterboxing runs on the
// GPU into the chunk's frame buffer.  Same three-stream pipeline as yolo2_hip_run_frames_int16:
// upload of chunk k+1 (CPU staging copy + DMA) overlaps the kernels of chunk k and the download of k-1.
// (channels: a Y2PixDesc::ch; pix: called from the _pix entry, where the camera and video formats are accepted)
static int run_images_i16_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights, int channels, bool pix,
                               int n, int batch, int16_t *region, int *final_q)
{
    if (!c || !images || !widths || !heights || !region) return fail(YOLO2_ERROR, "null argument");
    if (n <= 0 || batch <= 0) return fail(YOLO2_ERROR, "bad image count %d / batch %d", n, batch);
    if (!c->weights_loaded) return fail(YOLO2_ERROR, "weights not loaded");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    auto padded = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t table_bytes = padded((size_t)batch * sizeof(LetterboxItem));   // the chunk's letterbox table leads its staging buffer
    size_t cap = 0;   // bytes of the largest chunk
    for (int k = 0; k < chunks; ++k) {
        size_t sum = table_bytes;
        for (int i = k * batch; i < k * batch + in_chunk(k); ++i) {
            LetterboxArgs a;
            if (!images[i]) return fail(YOLO2_ERROR, "null image %d", i);
            const int rc = y2_letterbox_args(widths[i], heights[i], channels, 416, 416, a, pix);
            if (rc) return rc;
            sum += padded(y2_frame_bytes(widths[i], heights[i], channels));
        }
        cap = std::max(cap, sum);
    }
    if (batch != c->batch) {
        const int rc = yolo2_hip_set_batch(c, batch);
        if (rc) return rc;
    }
    const size_t rbytes = (size_t)batch * YOLO2_REGION_ELEMS * sizeof(int16_t);
    int rc = y2_pipe_ensure(c->pipe, cap, cap, batch);
    if (rc) return rc;
    PipeBufs &P = c->pipe;
    uint8_t *hin[2] = {P.hin[0].get(), P.hin[1].get()}, *dbytes[2] = {P.dbytes[0].get(), P.dbytes[1].get()};
    float *din[2] = {P.din[0].get(), P.din[1].get()};
    int16_t *hout[2] = {P.hout[0].get(), P.hout[1].get()}, *dout[2] = {P.dout[0].get(), P.dout[1].get()};
    hipStream_t s_in = P.s_in, s_run = P.s_run, s_out = P.s_out;
    hipEvent_t *e_in = P.e_in, *e_run = P.e_run, *e_out = P.e_out;
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)

    auto drain = [&](int k) {
        const int b = k & 1;
        (void)hipEventSynchronize(e_out[b]);
        memcpy(region + (size_t)k * batch * YOLO2_REGION_ELEMS, hout[b], (size_t)in_chunk(k) * YOLO2_REGION_ELEMS * sizeof(int16_t));
    };
    int q = 0;
    std::vector<size_t> offs((size_t)batch);
    for (int k = 0; k < chunks && rc == YOLO2_SUCCESS; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        if (k >= 2) drain(k - 2);   // buffer set b is free again once chunk k-2 has left it
        size_t off = table_bytes;
        for (int i = 0; i < nf; ++i) {
            const size_t bytes = y2_frame_bytes(widths[first + i], heights[first + i], channels);
            memcpy(hin[b] + off, images[first + i], bytes);
            offs[(size_t)i] = off;
            off += padded(bytes);
        }
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(hin[b]);
        for (int f = 0; f < batch && rc == YOLO2_SUCCESS; ++f) {   // a partial last chunk repeats its last image
            const int i = std::min(f, nf - 1);
            items[f].off = offs[(size_t)i];
            rc = y2_letterbox_args(widths[first + i], heights[first + i], channels, 416, 416, items[f].a, pix);
        }
        if (rc) break;
        Y2_TRY(hipMemcpyAsync(dbytes[b], hin[b], off, hipMemcpyHostToDevice, s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(e_in[b], s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(s_run, e_in[b], 0), YOLO2_ERROR);
        y2_launch_letterbox_batch(y2_ch_kind(channels), dbytes[b], din[b], batch, s_run);
        Y2_TRY(hipGetLastError(), YOLO2_ERROR);
        rc = yolo2_hip_run_batch_int16(c, (uint64_t)(uintptr_t)din[b], batch, (uint64_t)(uintptr_t)dout[b], &q, s_run);
        if (rc) break;
        Y2_TRY(hipEventRecord(e_run[b], s_run), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(s_out, e_run[b], 0), YOLO2_ERROR);
        Y2_TRY(hipMemcpyAsync(hout[b], dout[b], rbytes, hipMemcpyDeviceToHost, s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(e_out[b], s_out), YOLO2_ERROR);
    }
    if (rc == YOLO2_SUCCESS) {
        for (int k = std::max(0, chunks - 2); k < chunks; ++k) drain(k);
        if (final_q) *final_q = q;
    }
    cleanup();
#undef Y2_TRY
    return rc;
}

extern "C" int yolo2_hip_run_images_u8_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths,
                                            const int *heights, int channels, int n, int batch, int16_t *region,
                                            int *final_q)
{
    return run_images_i16_host(c, images, widths, heights, channels, false, n, batch, region, final_q);
}

extern "C" int yolo2_hip_run_images_pix_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                             int pixfmt, int n, int batch, int16_t *region, int *final_q)
{
    const int ch = pix_ch(pixfmt);
    return ch ? run_images_i16_host(c, images, widths, heights, ch, true, n, batch, region, final_q) : YOLO2_ERROR;
}

// Calibration from image bytes (yolo2_calib.hip has the statistics): the chunks and staging of the entry above - letterbox table +
// bytes H2D, one k_letterbox_*_batch launch - with y2_calib_frames in place of the int16 pass.  Chunk after chunk, no overlap:
// calibration runs once per weight set.  A short last chunk repeats its last image, which moves no maximum and is not counted.
extern "C" int yolo2_hip_calib_images_pix_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                               int pixfmt, int n, int batch)
{
    if (!c || !images || !widths || !heights) return fail(YOLO2_ERROR, "null argument");
    const int channels = pix_ch(pixfmt);
    if (!channels) return YOLO2_ERROR;
    if (n <= 0 || batch <= 0 || batch > 1024) return fail(YOLO2_ERROR, "bad image count %d / batch %d", n, batch);
    if (!c->f16_loaded || !c->wf32) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    auto padded = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t table_bytes = padded((size_t)batch * sizeof(LetterboxItem));
    size_t cap = 0;
    for (int k = 0; k < chunks; ++k) {
        size_t sum = table_bytes;
        for (int i = k * batch; i < k * batch + in_chunk(k); ++i) {
            LetterboxArgs a;
            if (!images[i]) return fail(YOLO2_ERROR, "null image %d", i);
            const int rc = y2_letterbox_args(widths[i], heights[i], channels, 416, 416, a, true);
            if (rc) return rc;
            sum += padded(y2_frame_bytes(widths[i], heights[i], channels));
        }
        cap = std::max(cap, sum);
    }
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    int rc = y2_pipe_ensure(c->pipe, cap, cap, batch, false);
    if (rc) return rc;
    PipeBufs &P = c->pipe;
    uint8_t *const hin = P.hin[0].get(), *const dbytes = P.dbytes[0].get();
    std::vector<size_t> offs((size_t)batch);
    for (int k = 0; k < chunks; ++k) {
        const int nf = in_chunk(k), first = k * batch;
        size_t off = table_bytes;
        for (int i = 0; i < nf; ++i) {
            const size_t bytes = y2_frame_bytes(widths[first + i], heights[first + i], channels);
            memcpy(hin + off, images[first + i], bytes);
            offs[(size_t)i] = off;
            off += padded(bytes);
        }
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(hin);
        for (int f = 0; f < batch; ++f) {
            const int i = std::min(f, nf - 1);
            items[f].off = offs[(size_t)i];
            if ((rc = y2_letterbox_args(widths[first + i], heights[first + i], channels, 416, 416, items[f].a, true))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(dbytes, hin, off, hipMemcpyHostToDevice, P.s_run), YOLO2_DMA_ERROR);
        y2_launch_letterbox_batch(y2_ch_kind(channels), dbytes, P.din[0].get(), batch, P.s_run);
        HIP_TRY(hipGetLastError(), YOLO2_ERROR);
        if ((rc = y2_calib_frames(c, (uint64_t)(uintptr_t)P.din[0].get(), batch, nf, P.s_run))) return rc;   // (synchronises: hin is free again)
    }
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- streaming host entry

// Camera-to-detections entry (the whole path incl. the step after it, at the path's rate): n images as host bytes -> detection
// records.  Per chunk of `batch` images: bytes H2D, letterbox + network on the device, the region tensor stays in HBM and
// region + boxes + NMS + record compaction run on the SAME device and stream right behind the network; only the records
// (32 bytes each) and the per-frame counts come back.  Upload of chunk k+1, kernels of chunk k and download of chunk k-1 overlap on
// three HIP streams.  Replaces the loop of the reference's streaming app (linux_app/src/main.c:878-1288), which runs
// yolo2_run_inference and the host post-processing frame by frame.
int y2_pipe_ensure_post(yolo2_hip_ctx *c, int batch, int cap)
{
    PipeBufs &p = c->pipe;
    if (p.post_batch >= batch && p.post_cap >= cap) return YOLO2_SUCCESS;
    batch = std::max(batch, p.post_batch);
    cap = std::max(cap, p.post_cap);
    for (int k = 0; k < 2; ++k) {
        p.hgeom[k].reset(); p.hdets[k].reset(); p.hcounts[k].reset();
        p.post_batch = p.post_cap = 0;
        const int rc = y2_post_alloc(c->device, batch, cap, &p.post[k]);
        if (rc) return rc;
        if (p.hgeom[k].alloc((size_t)batch * y2_post_geom_bytes()) || p.hdets[k].alloc((size_t)batch * cap) || p.hcounts[k].alloc((size_t)batch)) {
            (void)hipGetLastError();
            return fail(YOLO2_MMAP_ERROR, "pinned buffers for %d frames x %d detection records could not be allocated", batch, cap);
        }
    }
    p.post_batch = batch; p.post_cap = cap;
    return YOLO2_SUCCESS;
}

// (y2_internal.hpp) The int16 network of the chunk in buffer set b, for the entries that keep the region tensor in HBM: chunk letterbox
// on s_run (which already waits for the chunk's upload), then the network.  A chunk's lanes are NOT joined back into one stream here:
// consecutive chunks are independent, every lane owns its activations and its stream keeps its chunks in order, so lane i starts chunk
// k + 1 the moment it has finished chunk k (and the chunk's letterbox is done) instead of waiting for the slowest lane - the fork / join
// per 64 frames and the lanes' end spread (0.3 - 0.7 ms of a 20 ms step in the bench loop) do not exist in a stream of chunks.  Only what
// needs the whole region tensor waits for all of them: `done` receives the events to wait for.
int y2_pipe_enqueue_i16(yolo2_hip_ctx *c, int b, int kind, int batch, int *q, std::vector<hipEvent_t> *done)
{
    PipeBufs &P = c->pipe;
    done->clear();
    y2_launch_letterbox_batch(kind, P.dbytes[b].get(), P.din[b].get(), batch, P.s_run);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    bool own_streams = c->laned && (int)c->lanes.size() <= 8;
    if (own_streams) for (yolo2_hip_ctx *l : c->lanes) own_streams = own_streams && l->lane_stream;
    HIP_TRY(hipEventRecord(P.e_run[b], P.s_run), YOLO2_ERROR);            // (here: the letterboxed frames are ready)
    if (own_streams) {
        for (size_t i = 0; i < c->lanes.size(); ++i) {
            yolo2_hip_ctx *l = c->lanes[i];
            const uint64_t first = (uint64_t)c->lane_first[i];
            if (!P.e_lane[b][i]) HIP_TRY(hipEventCreateWithFlags(&P.e_lane[b][i], hipEventDisableTiming), YOLO2_ERROR);
            HIP_TRY(hipStreamWaitEvent(l->lane_stream, P.e_run[b], 0), YOLO2_ERROR);
            const int rc = yolo2_hip_run_batch_int16(l, (uint64_t)(uintptr_t)(P.din[b].get() + first * YOLO2_FRAME_ELEMS), l->batch,
                                                     (uint64_t)(uintptr_t)(P.dout[b].get() + first * YOLO2_REGION_ELEMS), q, l->lane_stream);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(P.e_lane[b][i], l->lane_stream), YOLO2_ERROR);
            done->push_back(P.e_lane[b][i]);
        }
    } else {
        const int rc = yolo2_hip_run_batch_int16(c, (uint64_t)(uintptr_t)P.din[b].get(), batch, (uint64_t)(uintptr_t)P.dout[b].get(), q, P.s_run);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(P.e_run[b], P.s_run), YOLO2_ERROR);
        done->push_back(P.e_run[b]);
    }
    return YOLO2_SUCCESS;
}

static int run_images_i16_dets(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights, int channels, bool pix,
                               int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap_per_frame, int *counts,
                               int *final_q)
{
    if (!c || !images || !widths || !heights || !dets || !counts) return fail(YOLO2_ERROR, "null argument");
    if (n <= 0 || batch <= 0 || cap_per_frame <= 0) return fail(YOLO2_ERROR, "bad image count %d / batch %d / capacity %d", n, batch, cap_per_frame);
    if (thresh < 0.f) return fail(YOLO2_ERROR, "negative threshold");
    if (!c->weights_loaded) return fail(YOLO2_ERROR, "weights not loaded");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch, cap = cap_per_frame, best_only = (flags & YOLO2_DETS_BEST_CLASS) ? 1 : 0,
              app_tail = (flags & YOLO2_DETS_APP_TAIL) ? 1 : 0;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    auto padded = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t table_bytes = padded((size_t)batch * sizeof(LetterboxItem));   // the chunk's letterbox table leads its staging buffer
    size_t cap_bytes = 0;   // bytes of the largest chunk
    for (int k = 0; k < chunks; ++k) {
        size_t sum = table_bytes;
        for (int i = k * batch; i < k * batch + in_chunk(k); ++i) {
            LetterboxArgs a;
            if (!images[i]) return fail(YOLO2_ERROR, "null image %d", i);
            const int rc = y2_letterbox_args(widths[i], heights[i], channels, 416, 416, a, pix);
            if (rc) return rc;
            sum += padded(y2_frame_bytes(widths[i], heights[i], channels));
        }
        cap_bytes = std::max(cap_bytes, sum);
    }
    if (batch != c->batch) {
        const int rc = yolo2_hip_set_batch(c, batch);
        if (rc) return rc;
    }
    int rc = y2_pipe_ensure(c->pipe, cap_bytes, cap_bytes, batch, false);
    if (rc == YOLO2_SUCCESS) rc = y2_pipe_ensure_post(c, batch, cap);
    if (rc) return rc;
    PipeBufs &P = c->pipe;
    const size_t gbytes = y2_post_geom_bytes();
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)
    auto drain = [&](int k) {
        const int b = k & 1, nf = in_chunk(k);
        (void)hipEventSynchronize(P.e_out[b]);
        memcpy(counts + (size_t)k * batch, P.hcounts[b].get(), (size_t)nf * sizeof(int));
        for (int f = 0; f < nf; ++f) {   // frame numbers are global in the caller's records
            const int cnt = std::min(P.hcounts[b].get()[f], cap);
            yolo2_hip_det *dst = dets + ((size_t)k * batch + f) * cap;
            memcpy(dst, P.hdets[b].get() + (size_t)f * cap, (size_t)cnt * sizeof(yolo2_hip_det));
            for (int r = 0; r < cnt; ++r) dst[r].frame = k * batch + f;
        }
    };
    int q = 0;
    std::vector<size_t> offs((size_t)batch);
    std::vector<int> cw((size_t)batch), chh((size_t)batch);
    std::vector<hipEvent_t> net_done;
    for (int k = 0; k < chunks && rc == YOLO2_SUCCESS; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        if (k >= 2) drain(k - 2);   // buffer set b is free again once chunk k-2 has left it
        size_t off = table_bytes;
        for (int i = 0; i < nf; ++i) {
            const size_t bytes = y2_frame_bytes(widths[first + i], heights[first + i], channels);
            memcpy(P.hin[b].get() + off, images[first + i], bytes);
            offs[(size_t)i] = off;
            off += padded(bytes);
        }
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(P.hin[b].get());
        for (int f = 0; f < batch; ++f) {   // a partial last chunk repeats its last image
            const int i = std::min(f, nf - 1);
            cw[(size_t)f] = widths[first + i]; chh[(size_t)f] = heights[first + i];
            items[f].off = offs[(size_t)i];
            if ((rc = y2_letterbox_args(widths[first + i], heights[first + i], channels, 416, 416, items[f].a, pix))) break;
        }
        if (rc) break;
        if ((rc = y2_post_fill_geom(P.hgeom[b].get(), cw.data(), chh.data(), batch))) break;
        Y2_TRY(hipMemcpyAsync(P.dbytes[b].get(), P.hin[b].get(), off, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipMemcpyAsync(P.post[b].geom.get(), P.hgeom[b].get(), (size_t)batch * gbytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_in[b], P.s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(P.s_run, P.e_in[b], 0), YOLO2_ERROR);
        if ((rc = y2_pipe_enqueue_i16(c, b, y2_ch_kind(channels), batch, &q, &net_done))) break;     // letterbox + network; lanes are not joined
        for (hipEvent_t e : net_done) Y2_TRY(hipStreamWaitEvent(P.s_out, e, 0), YOLO2_ERROR);
        // the step after the path, on the device that produced the tensor, straight from HBM - on the download stream, so that the
        // next chunk's letterbox and network need not wait for it (the tail is 64 workgroups for 0.7 ms: latency, not work)
        rc = y2_post_enqueue_int16(c->device, P.dout[b].get(), batch, q, thresh, nms, cap, best_only, app_tail, &P.post[b], P.s_out);
        if (rc) break;
        Y2_TRY(hipMemcpyAsync(P.hcounts[b].get(), P.post[b].counts.get(), (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipMemcpyAsync(P.hdets[b].get(), P.post[b].dets.get(), (size_t)batch * cap * sizeof(yolo2_hip_det), hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_out[b], P.s_out), YOLO2_ERROR);
    }
    if (rc == YOLO2_SUCCESS) {
        for (int k = std::max(0, chunks - 2); k < chunks; ++k) drain(k);
        if (final_q) *final_q = q;
    }
    cleanup();
#undef Y2_TRY
    return rc;
}

extern "C" int yolo2_hip_run_images_u8_dets(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                            int channels, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                            int cap_per_frame, int *counts, int *final_q)
{
    return run_images_i16_dets(c, images, widths, heights, channels, false, n, batch, thresh, nms, flags, dets, cap_per_frame, counts, final_q);
}

extern "C" int yolo2_hip_run_images_pix_dets(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                             int pixfmt, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                             int cap_per_frame, int *counts, int *final_q)
{
    const int ch = pix_ch(pixfmt);
    return ch ? run_images_i16_dets(c, images, widths, heights, ch, true, n, batch, thresh, nms, flags, dets, cap_per_frame, counts, final_q)
              : YOLO2_ERROR;
}

// ---------------------------------------------------------------------------- the fp16 / split-fp16 images entries
//
// yolo2_hip_run_images_u8_host / _dets on the matrix-core passes: the same chunks, staging format and three-stream overlap, but
// layers 0+1 read the chunk's bytes themselves (k_conv0_pool_mfma_u8: no letterboxed frame is written or read back), the region
// tensor is fp32 and the tail is y2_post_enqueue_f32.  Under f16_no_mfma0 the chunk is letterboxed into frames first and the frame
// path's table runs (the reference route the tests compare with).

int y2_pipe_ensure_regf(PipeBufs &p, int batch, bool need_host)
{
    if (p.regf_batch >= batch && (!need_host || p.hregf[0])) return YOLO2_SUCCESS;
    need_host = need_host || p.hregf[0];
    batch = std::max(batch, p.regf_batch);
    const size_t relems = (size_t)batch * YOLO2_REGION_ELEMS;
    for (int k = 0; k < 2; ++k) { p.hregf[k].reset(); p.dregf[k].reset(); }
    p.regf_batch = 0;
    for (int k = 0; k < 2; ++k)
        if (p.dregf[k].alloc(relems) || (need_host && p.hregf[k].alloc(relems))) {
            (void)hipGetLastError();
            return fail(YOLO2_MMAP_ERROR, "fp32 region buffers for %d frames could not be allocated", batch);
        }
    p.regf_batch = batch;
    return YOLO2_SUCCESS;
}

// The staging copy (pageable images -> the pinned chunk buffer) on up to kStageThreads threads: at the fp16 pass's rate one
// thread's memcpy would be the slowest stage of the pipeline.
static constexpr int kStageThreads = 4;

void y2_stage_images(uint8_t *dst, const uint8_t *const *images, const size_t *offs, const size_t *bytes, int nf)
{
    size_t total = 0;
    for (int i = 0; i < nf; ++i) total += bytes[i];
    const int nt = (int)std::min<size_t>(kStageThreads, std::max<size_t>(1, total >> 22));   // a thread per 4 MiB at most
    auto part = [&](int t) {   // an even share of the bytes; images are cut where the shares end
        const size_t lo = total * t / nt, hi = total * (t + 1) / nt;
        size_t at = 0;
        for (int i = 0; i < nf; ++i) {
            const size_t a = std::max(lo, at), b = std::min(hi, at + bytes[i]);
            if (a < b) memcpy(dst + offs[i] + (a - at), images[i] + (a - at), b - a);
            at += bytes[i];
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(part, t);
    part(0);
    for (auto &t : th) t.join();
}

// (y2_internal.hpp) The fp16 / split pass of the chunk in buffer set b on s_run, into dregf[b]: layers 0 + 1 from the chunk's bytes where
// the pass fuses them, else chunk letterbox + the frame path.  Records e_run[b] behind it.
int y2_pipe_enqueue_f16(yolo2_hip_ctx *c, yolo2_hip_ctx *run, bool fused, int b, int kind, int batch)
{
    PipeBufs &P = c->pipe;
    int rc;
    if (fused) {
        rc = y2_f16_run_images(run, P.dbytes[b].get(), kind, batch, P.dregf[b].get(), P.s_run);
    } else {
        y2_launch_letterbox_batch(kind, P.dbytes[b].get(), P.din[b].get(), batch, P.s_run);
        HIP_TRY(hipGetLastError(), YOLO2_ERROR);
        rc = yolo2_hip_run_batch_fp16(run, (uint64_t)(uintptr_t)P.din[b].get(), batch, (uint64_t)(uintptr_t)P.dregf[b].get(), P.s_run);
    }
    if (rc) return rc;
    HIP_TRY(hipEventRecord(P.e_run[b], P.s_run), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

// The chunk loop of the images entries whose pass leaves an fp32 region tensor (fp16, split-fp16, int8).
// dets == nullptr: region tensors to region_host; otherwise the records (the int16 dets entry's contract).
// resolve(): the pass's own refusals (weights not loaded ...), called after the argument checks and before anything is touched;
// enqueue(b, kind, batch): the network of the chunk in buffer set b on s_run into dregf[b], e_run[b] recorded behind it.
template <class Resolve, class Enqueue>
static int run_images_regf(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights, int channels, bool pix, int n,
                           int batch, float *region_host, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap, int *counts,
                           Resolve resolve, Enqueue enqueue)
{
    const bool want_dets = dets != nullptr;
    const int kind = y2_ch_kind(channels);
    if (n <= 0 || batch <= 0 || (want_dets && cap <= 0))
        return fail(YOLO2_ERROR, "bad image count %d / batch %d / capacity %d", n, batch, want_dets ? cap : 1);
    if (want_dets && thresh < 0.f) return fail(YOLO2_ERROR, "negative threshold");
    int rc = resolve();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    batch = std::min(batch, n);
    const int chunks = (n + batch - 1) / batch, best_only = (flags & YOLO2_DETS_BEST_CLASS) ? 1 : 0,
              app_tail = (flags & YOLO2_DETS_APP_TAIL) ? 1 : 0;
    auto in_chunk = [&](int k) { return std::min(batch, n - k * batch); };
    auto padded = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t table_bytes = padded((size_t)batch * sizeof(LetterboxItem));   // the chunk's letterbox table leads its staging buffer
    size_t cap_bytes = 0;   // bytes of the largest chunk
    for (int k = 0; k < chunks; ++k) {
        size_t sum = table_bytes;
        for (int i = k * batch; i < k * batch + in_chunk(k); ++i) {
            LetterboxArgs a;
            if (!images[i]) return fail(YOLO2_ERROR, "null image %d", i);
            if ((rc = y2_letterbox_args(widths[i], heights[i], channels, 416, 416, a, pix))) return rc;
            sum += padded(y2_frame_bytes(widths[i], heights[i], channels));
        }
        cap_bytes = std::max(cap_bytes, sum);
    }
    if ((rc = y2_pipe_ensure(c->pipe, cap_bytes, cap_bytes, batch, false))) return rc;      // (din: the frames of the f16_no_mfma0 / i8_no_front route)
    if ((rc = y2_pipe_ensure_regf(c->pipe, batch, !want_dets))) return rc;
    if (want_dets && (rc = y2_pipe_ensure_post(c, batch, cap))) return rc;
    PipeBufs &P = c->pipe;
    const size_t gbytes = y2_post_geom_bytes(), rbytes = (size_t)batch * YOLO2_REGION_ELEMS * sizeof(float);
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)
    auto drain = [&](int k) {
        const int b = k & 1, nf = in_chunk(k);
        (void)hipEventSynchronize(P.e_out[b]);
        if (!want_dets) {
            memcpy(region_host + (size_t)k * batch * YOLO2_REGION_ELEMS, P.hregf[b].get(), (size_t)nf * YOLO2_REGION_ELEMS * sizeof(float));
            return;
        }
        memcpy(counts + (size_t)k * batch, P.hcounts[b].get(), (size_t)nf * sizeof(int));
        for (int f = 0; f < nf; ++f) {   // frame numbers are global in the caller's records
            const int cnt = std::min(P.hcounts[b].get()[f], cap);
            yolo2_hip_det *dst = dets + ((size_t)k * batch + f) * cap;
            memcpy(dst, P.hdets[b].get() + (size_t)f * cap, (size_t)cnt * sizeof(yolo2_hip_det));
            for (int r = 0; r < cnt; ++r) dst[r].frame = k * batch + f;
        }
    };
    std::vector<size_t> offs((size_t)batch), sizes((size_t)batch);
    std::vector<int> cw((size_t)batch), chh((size_t)batch);
    for (int k = 0; k < chunks && rc == YOLO2_SUCCESS; ++k) {
        const int b = k & 1, nf = in_chunk(k), first = k * batch;
        if (k >= 2) drain(k - 2);   // buffer set b is free again once chunk k-2 has left it
        size_t off = table_bytes;
        for (int i = 0; i < nf; ++i) {
            sizes[(size_t)i] = y2_frame_bytes(widths[first + i], heights[first + i], channels);
            offs[(size_t)i] = off;
            off += padded(sizes[(size_t)i]);
        }
        y2_stage_images(P.hin[b].get(), images + first, offs.data(), sizes.data(), nf);
        LetterboxItem *items = reinterpret_cast<LetterboxItem *>(P.hin[b].get());
        for (int f = 0; f < batch; ++f) {   // a partial last chunk repeats its last image
            const int i = std::min(f, nf - 1);
            cw[(size_t)f] = widths[first + i]; chh[(size_t)f] = heights[first + i];
            items[f].off = offs[(size_t)i];
            if ((rc = y2_letterbox_args(widths[first + i], heights[first + i], channels, 416, 416, items[f].a, pix))) break;
        }
        if (rc) break;
        if (want_dets && (rc = y2_post_fill_geom(P.hgeom[b].get(), cw.data(), chh.data(), batch))) break;
        Y2_TRY(hipMemcpyAsync(P.dbytes[b].get(), P.hin[b].get(), off, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        if (want_dets) Y2_TRY(hipMemcpyAsync(P.post[b].geom.get(), P.hgeom[b].get(), (size_t)batch * gbytes, hipMemcpyHostToDevice, P.s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(P.e_in[b], P.s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(P.s_run, P.e_in[b], 0), YOLO2_ERROR);
        if ((rc = enqueue(b, kind, batch))) break;
        Y2_TRY(hipStreamWaitEvent(P.s_out, P.e_run[b], 0), YOLO2_ERROR);
        if (want_dets) {   // the tail on the download stream, straight from HBM (see yolo2_hip_run_images_u8_dets)
            if ((rc = y2_post_enqueue_f32(P.dregf[b].get(), batch, thresh, nms, cap, best_only, app_tail, &P.post[b], P.s_out))) break;
            Y2_TRY(hipMemcpyAsync(P.hcounts[b].get(), P.post[b].counts.get(), (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
            Y2_TRY(hipMemcpyAsync(P.hdets[b].get(), P.post[b].dets.get(), (size_t)batch * cap * sizeof(yolo2_hip_det), hipMemcpyDeviceToHost, P.s_out),
                   YOLO2_DMA_ERROR);
        } else {
            Y2_TRY(hipMemcpyAsync(P.hregf[b].get(), P.dregf[b].get(), rbytes, hipMemcpyDeviceToHost, P.s_out), YOLO2_DMA_ERROR);
        }
        Y2_TRY(hipEventRecord(P.e_out[b], P.s_out), YOLO2_ERROR);
    }
    if (rc == YOLO2_SUCCESS)
        for (int k = std::max(0, chunks - 2); k < chunks; ++k) drain(k);
    cleanup();
#undef Y2_TRY
    return rc;
}

static int run_images_f16(yolo2_hip_ctx *c, int split, const uint8_t *const *images, const int *widths, const int *heights, int channels,
                          bool pix, int n, int batch, float *region_host, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap,
                          int *counts)
{
    yolo2_hip_ctx *run = nullptr;
    bool fused = false;
    const int rc = run_images_regf(
        c, images, widths, heights, channels, pix, n, batch, region_host, thresh, nms, flags, dets, cap, counts,
        [&]() {
            const int r = y2_f16_images_ctx(c, split, &run);
            if (r == YOLO2_SUCCESS) fused = y2_f16_images_fused(run);
            return r;
        },
        [&](int b, int kind, int bt) { return y2_pipe_enqueue_f16(c, run, fused, b, kind, bt); });
    if (rc == YOLO2_SUCCESS)
        c->images_l0[split] = fused ? std::string(y2_f16_images_kernel(run, y2_ch_kind(channels)))
                                    : std::string(y2_letterbox_batch_kernel(y2_ch_kind(channels))) + " + " + yolo2_hip_fp16_layer_kernel(run, 0);
    return rc;
}

// ... and on the int8 pass (include/yolo2_hip.h "int8 pass"): k_i8_front_pix reads the chunk's bytes and writes layer 1's tensor; under
// i8_no_front the chunk is letterboxed into frames and the frames route runs (the reference route of the tests and the report).
static int run_images_i8(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights, int channels, int n, int batch,
                         float *region_host, float thresh, float nms, int flags, yolo2_hip_det *dets, int cap, int *counts)
{
    bool fused = false;
    const int rc = run_images_regf(
        c, images, widths, heights, channels, true, n, batch, region_host, thresh, nms, flags, dets, cap, counts,
        [&]() {
            if (!y2_i8_loaded(c)) return fail(YOLO2_ERROR, "int8 weights not loaded (yolo2_hip_load_weights_int8)");
            if (batch > 1024) return fail(YOLO2_ERROR, "batch %d out of range 1..1024", batch);
            fused = y2_i8_images_fused(c);
            return (int)YOLO2_SUCCESS;
        },
        [&](int b, int kind, int bt) {
            PipeBufs &P = c->pipe;
            int r;
            if (fused) {
                r = y2_i8_run_images(c, P.dbytes[b].get(), kind, bt, P.dregf[b].get(), P.s_run);
            } else {
                y2_launch_letterbox_batch(kind, P.dbytes[b].get(), P.din[b].get(), bt, P.s_run);
                HIP_TRY(hipGetLastError(), YOLO2_ERROR);
                r = yolo2_hip_run_batch_int8(c, (uint64_t)(uintptr_t)P.din[b].get(), bt, (uint64_t)(uintptr_t)P.dregf[b].get(), P.s_run);
            }
            if (r) return r;
            HIP_TRY(hipEventRecord(P.e_run[b], P.s_run), YOLO2_ERROR);
            return (int)YOLO2_SUCCESS;
        });
    if (rc == YOLO2_SUCCESS)
        c->images_front_i8 = fused ? std::string(y2_i8_front_kernel(y2_ch_kind(channels)))
                                   : std::string(y2_letterbox_batch_kernel(y2_ch_kind(channels))) + " + k_i8_quant_input + k_conv_i8";
    return rc;
}

extern "C" int yolo2_hip_run_images_pix_int8_host(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                                  int pixfmt, int n, int batch, float *region_host)
{
    if (!c || !images || !widths || !heights || !region_host) return fail(YOLO2_ERROR, "null argument");
    const int ch = pix_ch(pixfmt);
    return ch ? run_images_i8(c, images, widths, heights, ch, n, batch, region_host, 0.f, 0.f, 0, nullptr, 0, nullptr) : YOLO2_ERROR;
}

extern "C" int yolo2_hip_run_images_pix_dets_int8(yolo2_hip_ctx *c, const uint8_t *const *images, const int *widths, const int *heights,
                                                  int pixfmt, int n, int batch, float thresh, float nms, int flags, yolo2_hip_det *dets,
                                                  int cap_per_frame, int *counts)
{
    if (!c || !images || !widths || !heights || !dets || !counts) return fail(YOLO2_ERROR, "null argument");
    const int ch = pix_ch(pixfmt);
    return ch ? run_images_i8(c, images, widths, heights, ch, n, batch, nullptr, thresh, nms, flags, dets, cap_per_frame, counts) : YOLO2_ERROR;
}

extern "C" const char *yolo2_hip_images_front_kernel_int8(yolo2_hip_ctx *c) { return c ? c->images_front_i8.c_str() : ""; }

extern "C" int yolo2_hip_run_images_u8_f16_host(yolo2_hip_ctx *c, int split, const uint8_t *const *images, const int *widths,
                                                const int *heights, int channels, int n, int batch, float *region_host)
{
    if (!c || !images || !widths || !heights || !region_host) return fail(YOLO2_ERROR, "null argument");
    return run_images_f16(c, split, images, widths, heights, channels, false, n, batch, region_host, 0.f, 0.f, 0, nullptr, 0, nullptr);
}

extern "C" int yolo2_hip_run_images_pix_f16_host(yolo2_hip_ctx *c, int split, const uint8_t *const *images, const int *widths,
                                                 const int *heights, int pixfmt, int n, int batch, float *region_host)
{
    if (!c || !images || !widths || !heights || !region_host) return fail(YOLO2_ERROR, "null argument");
    const int ch = pix_ch(pixfmt);
    return ch ? run_images_f16(c, split, images, widths, heights, ch, true, n, batch, region_host, 0.f, 0.f, 0, nullptr, 0, nullptr) : YOLO2_ERROR;
}

extern "C" int yolo2_hip_run_images_u8_dets_f16(yolo2_hip_ctx *c, int split, const uint8_t *const *images, const int *widths,
                                                const int *heights, int channels, int n, int batch, float thresh, float nms, int flags,
                                                yolo2_hip_det *dets, int cap_per_frame, int *counts)
{
    if (!c || !images || !widths || !heights || !dets || !counts) return fail(YOLO2_ERROR, "null argument");
    return run_images_f16(c, split, images, widths, heights, channels, false, n, batch, nullptr, thresh, nms, flags, dets, cap_per_frame, counts);
}

extern "C" int yolo2_hip_run_images_pix_dets_f16(yolo2_hip_ctx *c, int split, const uint8_t *const *images, const int *widths,
                                                 const int *heights, int pixfmt, int n, int batch, float thresh, float nms, int flags,
                                                 yolo2_hip_det *dets, int cap_per_frame, int *counts)
{
    if (!c || !images || !widths || !heights || !dets || !counts) return fail(YOLO2_ERROR, "null argument");
    const int ch = pix_ch(pixfmt);
    return ch ? run_images_f16(c, split, images, widths, heights, ch, true, n, batch, nullptr, thresh, nms, flags, dets, cap_per_frame, counts)
              : YOLO2_ERROR;
}

extern "C" const char *yolo2_hip_images_layer0_kernel(yolo2_hip_ctx *c, int split)
{
    return c && (split == 0 || split == 1) ? c->images_l0[split].c_str() : "";
}

extern "C" int yolo2_hip_run_frames_int16(yolo2_hip_ctx *c, const float *frames, int n_frames, int batch, int16_t *region,
                                          int *final_q)
{
    if (!c || !frames || !region) return fail(YOLO2_ERROR, "null argument");
    if (n_frames <= 0 || batch <= 0) return fail(YOLO2_ERROR, "bad frame count / batch");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    if (batch != c->batch) {
        const int rc = yolo2_hip_set_batch(c, batch);
        if (rc) return rc;
    }
    const size_t fbytes = (size_t)batch * YOLO2_FRAME_ELEMS * sizeof(float), rbytes = (size_t)batch * YOLO2_REGION_ELEMS * sizeof(int16_t);
    int rc = y2_pipe_ensure(c->pipe, fbytes, 0, batch);
    if (rc) return rc;
    PipeBufs &P = c->pipe;
    float *hin[2] = {(float *)P.hin[0].get(), (float *)P.hin[1].get()}, *din[2] = {P.din[0].get(), P.din[1].get()};
    int16_t *hout[2] = {P.hout[0].get(), P.hout[1].get()}, *dout[2] = {P.dout[0].get(), P.dout[1].get()};
    hipStream_t s_in = P.s_in, s_run = P.s_run, s_out = P.s_out;
    hipEvent_t *e_in = P.e_in, *e_run = P.e_run, *e_out = P.e_out;
    auto cleanup = [&]() { (void)hipDeviceSynchronize(); };
#define Y2_TRY(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail(code, "%s failed: %s", #expr, hipGetErrorString(e_)); cleanup(); return rc; } } while (0)

    const int chunks = (n_frames + batch - 1) / batch;
    auto frames_in_chunk = [&](int k) { return std::min(batch, n_frames - k * batch); };
    auto drain = [&](int k) {   // copy chunk k's results from its pinned buffer to the caller's memory
        const int b = k & 1;
        (void)hipEventSynchronize(e_out[b]);
        memcpy(region + (size_t)k * batch * YOLO2_REGION_ELEMS, hout[b], (size_t)frames_in_chunk(k) * YOLO2_REGION_ELEMS * sizeof(int16_t));
    };
    int q = 0;
    for (int k = 0; k < chunks && rc == YOLO2_SUCCESS; ++k) {
        const int b = k & 1, nf = frames_in_chunk(k);
        if (k >= 2) drain(k - 2);   // buffer set b is free again once chunk k-2 has left it
        // stage: pageable -> pinned (CPU), pad a partial last chunk with its last frame
        memcpy(hin[b], frames + (size_t)k * batch * YOLO2_FRAME_ELEMS, (size_t)nf * YOLO2_FRAME_ELEMS * sizeof(float));
        for (int f = nf; f < batch; ++f)
            memcpy(hin[b] + (size_t)f * YOLO2_FRAME_ELEMS, hin[b] + (size_t)(nf - 1) * YOLO2_FRAME_ELEMS, YOLO2_FRAME_ELEMS * sizeof(float));
        Y2_TRY(hipMemcpyAsync(din[b], hin[b], fbytes, hipMemcpyHostToDevice, s_in), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(e_in[b], s_in), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(s_run, e_in[b], 0), YOLO2_ERROR);
        rc = yolo2_hip_run_batch_int16(c, (uint64_t)(uintptr_t)din[b], batch, (uint64_t)(uintptr_t)dout[b], &q, s_run);
        if (rc) break;
        Y2_TRY(hipEventRecord(e_run[b], s_run), YOLO2_ERROR);
        Y2_TRY(hipStreamWaitEvent(s_out, e_run[b], 0), YOLO2_ERROR);
        Y2_TRY(hipMemcpyAsync(hout[b], dout[b], rbytes, hipMemcpyDeviceToHost, s_out), YOLO2_DMA_ERROR);
        Y2_TRY(hipEventRecord(e_out[b], s_out), YOLO2_ERROR);
    }
    if (rc == YOLO2_SUCCESS) {
        for (int k = std::max(0, chunks - 2); k < chunks; ++k) drain(k);
        if (final_q) *final_q = q;
    }
    cleanup();
#undef Y2_TRY
    return rc;
}
