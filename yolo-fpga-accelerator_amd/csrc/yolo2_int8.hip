// yolo2_int8.hip -- the int8 pass (include/yolo2_hip.h "int8 pass"): the weight quantiser, the loader with its
// refusals and the device-side weight packing, run_batch_int8, the parity hook and the driver tier's single-layer device work.
// One stream, no lanes; every launch is in this file (kernels_i8.hpp, kernels_i8_front.hpp).  y2_i8_run_images is the pass from a
// chunk of image bytes: k_i8_front_pix into layer 1's tensor, then the frames route's layers 2..30.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "y2_internal.hpp"
#include "kernels_i8.hpp"
#include "kernels_i8_front.hpp"
#include "kernels_i8_front_pix.hpp"

using namespace y2;

struct Y2I8Tensor {
    signed char *d = nullptr;        // channel 0 of the tensor (a view starts at its channel offset inside the owner)
    Y2DevBuf<signed char> own;
    int C = 0, cs = 0, H = 0, W = 0, q = 0;   // cs: bytes between pixels (a multiple of 32)
};

struct Y2I8 {
    bool loaded = false;
    int act_q[YOLO2_N_CONV + 1] = {};
    Y2DevBuf<signed char> wpk;       // all layers, [tap][chunk][Np][32] each
    Y2DevBuf<signed char> w0front;   // layer 0 again as k_i8_front_pix's A fragments (front_pack_weights, 1 KB)
    Y2DevBuf<int> bias, sh;          // all layers, padded to Np each
    long wpk_off[YOLO2_N_CONV] = {}, ch_off[YOLO2_N_CONV] = {};
    int Np[YOLO2_N_CONV] = {};
    int batch = 0, last_batch = 0;
    bool front_tensors = false;      // t_in and t[0] are allocated (the frames route; the images route never touches them)
    bool last_fused = false;         // the last run wrote t[1] with k_i8_front_pix: t_in and t[0] hold nothing of it
    Y2I8Tensor t_in, t[32];
};

void y2_i8_free(yolo2_hip_ctx *c)
{
    delete c->i8;
    c->i8 = nullptr;
}

namespace {

constexpr int kQMin = -8, kQMax = 24, kSMin = -7, kSMax = 31;

// output channels per workgroup of the conv launch for a layer of N output channels (the weights are padded to a multiple of it)
int tile_m(int N) { return N <= 32 ? 32 : (N <= 64 ? 64 : 128); }

// Q of the tensor conv ordinal `ord` reads
int qin_of(int ord, const int32_t *act_q) { return act_q[y2_act_q_slot(kWire[kConvLayer[ord]].src)]; }

void launch_conv(const ConvI8Args &a, bool fout, hipStream_t st)
{
    const int bm = tile_m(a.N), bp = bm == 128 ? 128 : 256;
    const dim3 grid(blocks_for(a.P, bp), a.Np / bm), block(256);
    if (bm == 32) {
        if (fout) hipLaunchKernelGGL((k_conv_i8<1, 1, 2, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_conv_i8<1, 1, 2, false>), grid, block, 0, st, a);
    } else if (bm == 64) {
        if (fout) hipLaunchKernelGGL((k_conv_i8<1, 2, 2, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_conv_i8<1, 2, 2, false>), grid, block, 0, st, a);
    } else {
        if (fout) hipLaunchKernelGGL((k_conv_i8<2, 2, 2, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_conv_i8<2, 2, 2, false>), grid, block, 0, st, a);
    }
}

// The refusals of one layer, on host arrays: Q ranges, the shift range (int8 output only) and the 32-bit proof per output channel.
// sh_out[N] receives what the kernel's epilogue takes: s, or Qin + Qw for a float output.
int check_layer(const char *what, const int8_t *w, const int32_t *bias, const int32_t *qw, int N, long per, int qin, int qout, bool fout,
                int *sh_out)
{
    if (qin < kQMin || qin > kQMax) return fail(YOLO2_ERROR, "%s: input Q %d outside %d..%d", what, qin, kQMin, kQMax);
    if (!fout && (qout < kQMin || qout > kQMax)) return fail(YOLO2_ERROR, "%s: output Q %d outside %d..%d", what, qout, kQMin, kQMax);
    for (int m = 0; m < N; ++m) {
        if (qw[m] < kQMin || qw[m] > kQMax) return fail(YOLO2_ERROR, "%s, channel %d: weight Q %d outside %d..%d", what, m, qw[m], kQMin, kQMax);
        const int s = qin + qw[m] - (fout ? 0 : qout);
        if (!fout && (s < kSMin || s > kSMax))
            return fail(YOLO2_ERROR, "%s, channel %d: shift s = %d + %d - %d = %d outside %d..%d", what, m, qin, qw[m], qout, s, kSMin, kSMax);
        long sum = 0;
        const int8_t *wm = w + (long)m * per;
        for (long e = 0; e < per; ++e) sum += wm[e] < 0 ? -(long)wm[e] : (long)wm[e];
        const long b = bias[m] < 0 ? -(long)bias[m] : (long)bias[m];
        if (b + 128 * sum + (1l << 30) >= (1l << 31))
            return fail(YOLO2_ERROR, "%s, channel %d: |bias32| + 128 * sum|w8| + 2^30 = %ld does not stay below 2^31 (32-bit accumulator proof)", what,
                        m, b + 128 * sum + (1l << 30));
        sh_out[m] = s;
    }
    return YOLO2_SUCCESS;
}

void launch_pack_weights(const signed char *w_nat, signed char *out, int N, int C, int K, int Np, hipStream_t st)
{
    const int CC = (C + 31) / 32;
    const long n = (long)K * K * CC * Np * 32;
    hipLaunchKernelGGL(k_i8_pack_weights, dim3(blocks_for(n, 256)), dim3(256), 0, st, w_nat, out, N, C, K * K, CC, Np, n);
}

int need_i8(const yolo2_hip_ctx *c)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    if (!c->i8 || !c->i8->loaded) return fail(YOLO2_ERROR, "int8 weights not loaded (yolo2_hip_load_weights_int8)");
    return YOLO2_SUCCESS;
}

// the activation tensors of the pass for `batch` frames (kept until the batch or the weight set changes).  front: with the quantised
// input and layer 0's tensor (2 * batch * 416 * 416 * 32 bytes), which only the frames route reads and writes: they are allocated at
// the first frames run at this batch.
int ensure_tensors(Y2I8 *s, int batch, bool front)
{
    int rc;
    if (s->batch == batch) {
        if (front && !s->front_tensors) {
            for (Y2I8Tensor *t : {&s->t_in, &s->t[0]})
                if ((rc = y2_alloc_owned(t->own, t->d, (size_t)batch * t->H * t->W * t->cs))) return rc;
            s->front_tensors = true;
        }
        return YOLO2_SUCCESS;
    }
    s->batch = 0;
    s->front_tensors = false;
    auto make = [&](Y2I8Tensor &t, int C, int H, int W, int q) {
        t.C = C; t.cs = round_up(C, kI8Granule); t.H = H; t.W = W; t.q = q;
        if (!front && (&t == &s->t_in || &t == &s->t[0])) {   // geometry only
            t.own.reset();
            t.d = nullptr;
            return (int)YOLO2_SUCCESS;
        }
        return y2_alloc_owned(t.own, t.d, (size_t)batch * H * W * t.cs);
    };
    auto view = [&](Y2I8Tensor &t, const Y2I8Tensor &of, int ch0, int C, int q) {
        t.own.reset();
        t.d = of.d + ch0; t.C = C; t.cs = of.cs; t.H = of.H; t.W = of.W; t.q = q;
    };
    if ((rc = make(s->t_in, kNet[0].c, kNet[0].h, kNet[0].w, s->act_q[0]))) return rc;
    const int cat = kWire[kWiring.cat_conv].cat;   // the concat tensor: its route layer's slot, the members are views into it
    if ((rc = make(s->t[cat], kWire[cat].C, kWire[cat].H, kWire[cat].W, s->act_q[y2_act_q_slot(cat)]))) return rc;
    for (int i = 0; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        const NetWire &w = kWire[i];
        Y2I8Tensor &t = s->t[i];
        const int q = s->act_q[y2_act_q_slot(l.type == L_CONV ? i : w.src)];   // a conv's own, otherwise its input's
        if (w.to_region || l.type == L_REGION || i == cat) continue;
        if (w.cat >= 0) view(t, s->t[cat], w.ch_off, l.n, q);
        else if (l.type == L_ROUTE) view(t, s->t[w.src], 0, s->t[w.src].C, s->t[w.src].q);
        else if ((rc = make(t, w.C, w.H, w.W, q))) return rc;
    }
    s->batch = batch;
    s->front_tensors = front;
    return YOLO2_SUCCESS;
}

// layers first..30 of the pass on `cur` (the tensor layer `first` reads), shared by the frames route (first = 0) and the images
// route (first = 2); ev[i + 1] is recorded behind layer i
int run_layers(Y2I8 *s, int first, const Y2I8Tensor *cur, int batch, uint64_t region_dev, hipStream_t st, hipEvent_t *ev)
{
    for (int i = first; i < 32; ++i) {
        const LayerDesc &l = kNet[i];
        if (l.type == L_CONV) {
            if (cur->C != l.c || cur->H != l.h || cur->W != l.w) return fail(YOLO2_ERROR, "int8 pass: layer %d does not fit the tensor it reads", i);
            const int ord = kWire[i].ord;
            ConvI8Args a;
            a.in = cur->d;
            a.w = s->wpk.get() + s->wpk_off[ord];
            a.bias = s->bias.get() + s->ch_off[ord];
            a.sh = s->sh.get() + s->ch_off[ord];
            a.CC = cur->cs / 32;
            a.K = l.size; a.H = l.h; a.W = l.w; a.P = batch * l.h * l.w;
            a.N = l.n; a.Np = s->Np[ord]; a.leaky = l.leaky;
            if (kWire[i].to_region) {
                a.out = (void *)(uintptr_t)region_dev;
                a.ocs = 0;
            } else {
                a.out = s->t[i].d;
                a.ocs = s->t[i].cs;
                cur = &s->t[i];
            }
            launch_conv(a, kWire[i].to_region, st);
        } else if (l.type == L_MAX) {
            const long n = (long)batch * (l.h / 2) * (l.w / 2) * (cur->cs / 16);
            hipLaunchKernelGGL(k_i8_pool, dim3(blocks_for(n, 256)), dim3(256), 0, st, (const signed char *)cur->d, s->t[i].d, l.h, l.w, cur->cs, n);
            cur = &s->t[i];
        } else if (l.type == L_ROUTE) {
            cur = &s->t[i];
        } else if (l.type == L_REORG) {
            hipLaunchKernelGGL(k_i8_reorg, dim3(blocks_for((long)batch * 256 * 169, 256)), dim3(256), 0, st, (const signed char *)cur->d, s->t[i].d, batch,
                               cur->cs, s->t[i].cs);
            cur = &s->t[i];
        }
        if (ev) (void)hipEventRecord(ev[i + 1], st);
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    return YOLO2_SUCCESS;
}

}  // namespace

// ---------------------------------------------------------------------------- quantiser

extern "C" int yolo2_hip_quantize_weights_int8(yolo2_hip_ctx *c, const int32_t *act_q, int8_t *w8_out, size_t n_w, int32_t *bias32_out, size_t n_b,
                                               int32_t *weight_q_out)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    if (!c->f16_loaded || !c->wf32 || !c->bf32) return fail(YOLO2_ERROR, "fp32 weights not loaded (yolo2_hip_load_weights_fp32)");
    if (!act_q || !w8_out || !bias32_out || !weight_q_out) return fail(YOLO2_ERROR, "null argument");
    if (n_w < (size_t)YOLO2_N_WEIGHTS || n_b < (size_t)YOLO2_N_BIAS)
        return fail(YOLO2_ERROR, "output buffers of %zu / %zu elements are short of %d weights / %d channels", n_w, n_b, YOLO2_N_WEIGHTS, YOLO2_N_BIAS);
    for (int i = 0; i <= YOLO2_N_CONV; ++i)
        if (act_q[i] < kQMin || act_q[i] > kQMax) return fail(YOLO2_ERROR, "act_q[%d] = %d outside %d..%d", i, act_q[i], kQMin, kQMax);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    Y2DevBuf<signed char> w8;
    Y2DevBuf<int> b32, qw;
    int rc;
    if ((rc = w8.alloc(YOLO2_N_WEIGHTS)) || (rc = b32.alloc(YOLO2_N_BIAS)) || (rc = qw.alloc(YOLO2_N_BIAS))) return rc;
    for (int ord = 0; ord < YOLO2_N_CONV; ++ord) {
        const LayerDesc &l = kNet[kConvLayer[ord]];
        const long woff = kWire[kConvLayer[ord]].w_off, boff = kWire[kConvLayer[ord]].b_off;
        hipLaunchKernelGGL(k_quantize_i8, dim3(l.n), dim3(256), 0, nullptr, (const float *)(c->wf32 + woff), (const float *)(c->bf32 + boff),
                           w8.get() + woff, b32.get() + boff, qw.get() + boff, l.n, l.c, l.size * l.size, qin_of(ord, act_q));
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpy(w8_out, w8.get(), (size_t)YOLO2_N_WEIGHTS, hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(bias32_out, b32.get(), (size_t)YOLO2_N_BIAS * sizeof(int32_t), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(weight_q_out, qw.get(), (size_t)YOLO2_N_BIAS * sizeof(int32_t), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    for (int o = 0; o < YOLO2_N_CONV; ++o)
        for (int m = 0; m < yolo2_bias_len[o]; ++m)
            if (weight_q_out[kWire[kConvLayer[o]].b_off + m] == kI8NoQ)
                return fail(YOLO2_ERROR, "no Q in %d..%d holds the weights of conv %d, channel %d (or one of them is not finite)", kQMin, kQMax, o, m);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- loader

extern "C" int yolo2_hip_load_weights_int8(yolo2_hip_ctx *c, const int8_t *w8, size_t n_w, const int32_t *bias32, size_t n_b, const int32_t *weight_q,
                                           const int32_t *act_q)
{
    if (!c) return fail(YOLO2_ERROR, "null ctx");
    if (!w8 || !bias32 || !weight_q || !act_q) return fail(YOLO2_ERROR, "null argument");
    if (n_w != (size_t)YOLO2_N_WEIGHTS || n_b != (size_t)YOLO2_N_BIAS)
        return fail(YOLO2_ERROR, "int8 weight set of %zu weights / %zu channels, the network has %d / %d", n_w, n_b, YOLO2_N_WEIGHTS, YOLO2_N_BIAS);
    for (int i = 0; i <= YOLO2_N_CONV; ++i)
        if (act_q[i] < kQMin || act_q[i] > kQMax) return fail(YOLO2_ERROR, "act_q[%d] = %d outside %d..%d", i, act_q[i], kQMin, kQMax);
    const int q_conv = kWire[kWiring.cat_conv].ord + 1, q_feed = kWire[kWiring.cat_feed].ord + 1;
    if (act_q[q_conv] != act_q[q_feed])
        return fail(YOLO2_ERROR, "act_q[%d] = %d (layer %d) and act_q[%d] = %d (layer %d) differ: the concat tensor of layer %d needs one Q", q_conv,
                    act_q[q_conv], kWiring.cat_conv, q_feed, act_q[q_feed], kWiring.cat_feed, kWire[kWire[kWiring.cat_conv].cat].reader);
    // every refusal on the host, before anything is allocated or launched
    std::vector<int> sh_host;
    long wpk_off[YOLO2_N_CONV], ch_off[YOLO2_N_CONV], wtot = 0, ctot = 0;
    int Np[YOLO2_N_CONV];
    {
        for (int ord = 0; ord < YOLO2_N_CONV; ++ord) {
            const int i = kConvLayer[ord];
            const LayerDesc &l = kNet[i];
            const long woff = kWire[i].w_off, boff = kWire[i].b_off;
            Np[ord] = round_up(l.n, tile_m(l.n));
            wpk_off[ord] = wtot;
            ch_off[ord] = ctot;
            wtot += (long)l.size * l.size * ((l.c + 31) / 32) * Np[ord] * 32;
            ctot += Np[ord];
            sh_host.resize(ctot, 0);
            char what[48];
            snprintf(what, sizeof(what), "conv %d (layer %d)", ord, i);
            const int rc = check_layer(what, w8 + woff, bias32 + boff, weight_q + boff, l.n, (long)l.c * l.size * l.size, qin_of(ord, act_q),
                                       act_q[ord + 1], kWire[i].to_region, sh_host.data() + ch_off[ord]);
            if (rc) return rc;
        }
    }
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);   // a run in flight reads what is replaced below
    if (!c->i8) c->i8 = new Y2I8;
    Y2I8 *s = c->i8;
    s->loaded = false;
    s->batch = 0;
    s->last_batch = 0;
    int rc;
    Y2DevBuf<signed char> nat;
    if ((rc = nat.alloc(YOLO2_N_WEIGHTS)) || (rc = s->wpk.alloc(wtot)) || (rc = s->w0front.alloc(32 * 32)) || (rc = s->bias.alloc(ctot)) ||
        (rc = s->sh.alloc(ctot)))
        return rc;
    HIP_TRY(hipMemcpy(nat.get(), w8, (size_t)YOLO2_N_WEIGHTS, hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    {   // layer 0 (the first 32 * 27 of w8) in the front kernel's fragment order, from the same natural-order bytes
        int8_t front[32 * 32];
        front_pack_weights(w8, front);
        HIP_TRY(hipMemcpy(s->w0front.get(), front, sizeof(front), hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    }
    std::vector<int> bias_host(ctot, 0);
    for (int ord = 0; ord < YOLO2_N_CONV; ++ord) {
        const LayerDesc &l = kNet[kConvLayer[ord]];
        memcpy(bias_host.data() + ch_off[ord], bias32 + kWire[kConvLayer[ord]].b_off, (size_t)l.n * sizeof(int));
        launch_pack_weights(nat.get() + kWire[kConvLayer[ord]].w_off, s->wpk.get() + wpk_off[ord], l.n, l.c, l.size, Np[ord], nullptr);
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpy(s->bias.get(), bias_host.data(), (size_t)ctot * sizeof(int), hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(s->sh.get(), sh_host.data(), (size_t)ctot * sizeof(int), hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);   // `nat` is freed on return
    memcpy(s->act_q, act_q, sizeof(s->act_q));
    memcpy(s->wpk_off, wpk_off, sizeof(wpk_off));
    memcpy(s->ch_off, ch_off, sizeof(ch_off));
    memcpy(s->Np, Np, sizeof(Np));
    s->loaded = true;
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- the pass

extern "C" int yolo2_hip_run_batch_int8(yolo2_hip_ctx *c, uint64_t frames_dev, int batch, uint64_t region_dev, void *stream)
{
    int rc = need_i8(c);
    if (rc) return rc;
    if (!frames_dev || !region_dev) return fail(YOLO2_ERROR, "null buffer address");
    if ((frames_dev & 3) || (region_dev & 3)) return fail(YOLO2_ERROR, "frames and region tensor start on a 4-byte boundary");
    if (batch <= 0 || batch > 1024) return fail(YOLO2_ERROR, "batch %d out of range 1..1024", batch);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    Y2I8 *s = c->i8;
    hipStream_t st = (hipStream_t)stream;
    if (s->batch != batch) HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);   // the tensors of the previous batch may still be read
    if ((rc = ensure_tensors(s, batch, true))) return rc;
    if (c->prof && (rc = y2_ensure_prof_events(c))) return rc;
    hipEvent_t *ev = c->prof ? c->ev[c->prof_runs % yolo2_hip_ctx::kProfSlots] : nullptr;
    {
        const long n = (long)batch * 416 * 416;
        hipLaunchKernelGGL(k_i8_quant_input, dim3(blocks_for(n, 256)), dim3(256), 0, st, (const float *)(uintptr_t)frames_dev, s->t_in.d,
                           s->act_q[0], 416 * 416, n);
    }
    if (ev) HIP_TRY(hipEventRecord(ev[0], st), YOLO2_ERROR);
    if ((rc = run_layers(s, 0, &s->t_in, batch, region_dev, st, ev))) return rc;
    if (ev) c->prof_runs++;
    s->last_batch = batch;
    s->last_fused = false;
    return YOLO2_SUCCESS;
}

// (y2_internal.hpp) The pass on a chunk of `batch` images whose staging buffer is at lb: the front kernel into layer 1's tensor, then
// layers 2..30.  Profiling: the front's time is layer 1's slot (ev[1] .. ev[2]); layer 0's slot is empty.
bool y2_i8_loaded(const yolo2_hip_ctx *c) { return c && c->i8 && c->i8->loaded; }
bool y2_i8_images_fused(const yolo2_hip_ctx *c) { return !c->opt.i8_no_front; }
const char *y2_i8_front_kernel(int kind)
{
    static const char *const names[Y2_KIND_COUNT] = {"k_i8_front_u8",    "k_i8_front_yuyv",   "k_i8_front_nv12",  "k_i8_front_i420",
                                                     "k_i8_front_bgr24", "k_i8_front_rgba32", "k_i8_front_bgra32"};
    return names[kind];
}

int y2_i8_run_images(yolo2_hip_ctx *c, const uint8_t *lb, int kind, int batch, float *region_dev, hipStream_t st)
{
    int rc = need_i8(c);
    if (rc) return rc;
    if (!lb || !region_dev) return fail(YOLO2_ERROR, "null buffer address");
    if (batch <= 0 || batch > 1024) return fail(YOLO2_ERROR, "batch %d out of range 1..1024", batch);
    Y2I8 *s = c->i8;
    if (s->batch != batch) HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);   // the tensors of the previous batch may still be read
    if ((rc = ensure_tensors(s, batch, false))) return rc;
    if (c->prof && (rc = y2_ensure_prof_events(c))) return rc;
    hipEvent_t *ev = c->prof ? c->ev[c->prof_runs % yolo2_hip_ctx::kProfSlots] : nullptr;
    if (ev) {
        HIP_TRY(hipEventRecord(ev[0], st), YOLO2_ERROR);
        HIP_TRY(hipEventRecord(ev[1], st), YOLO2_ERROR);
    }
    FrontI8Args a;
    a.lb = lb;
    a.w = s->w0front.get();
    a.bias = s->bias.get() + s->ch_off[0];
    a.sh = s->sh.get() + s->ch_off[0];
    a.out = s->t[1].d;
    a.q0 = s->act_q[0];
    a.leaky = kNet[0].leaky;
    const dim3 grid((unsigned)batch * kFrontTilesPerFrame), block(256);
    if (kind == Y2_KIND_YUYV) hipLaunchKernelGGL(k_i8_front_pix<LbYuyv>, grid, block, 0, st, a);
    else if (kind == Y2_KIND_NV12) hipLaunchKernelGGL(k_i8_front_nv12, grid, block, 0, st, a);
    else if (kind == Y2_KIND_I420) hipLaunchKernelGGL(k_i8_front_i420, grid, block, 0, st, a);
    else if (kind == Y2_KIND_BGR24) hipLaunchKernelGGL(k_i8_front_bgr24, grid, block, 0, st, a);
    else if (kind == Y2_KIND_RGBA32) hipLaunchKernelGGL(k_i8_front_rgba32, grid, block, 0, st, a);
    else if (kind == Y2_KIND_BGRA32) hipLaunchKernelGGL(k_i8_front_bgra32, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_i8_front_pix<LbInterleaved>, grid, block, 0, st, a);
    if (ev) (void)hipEventRecord(ev[2], st);
    if ((rc = run_layers(s, 2, &s->t[1], batch, (uint64_t)(uintptr_t)region_dev, st, ev))) return rc;
    if (ev) c->prof_runs++;
    s->last_batch = batch;
    s->last_fused = true;
    return YOLO2_SUCCESS;
}

extern "C" int yolo2_hip_run_batch_int8_host(yolo2_hip_ctx *c, const float *frames, int batch, float *region)
{
    const int rc0 = need_i8(c);
    if (rc0) return rc0;
    if (batch <= 0 || batch > 1024) return fail(YOLO2_ERROR, "batch %d out of range 1..1024", batch);
    return y2_run_batch_host<float>(c, frames, batch, region,
                                    [&](uint64_t f, uint64_t r) { return yolo2_hip_run_batch_int8(c, f, batch, r, nullptr); });
}

extern "C" int yolo2_hip_debug_i8_tensor(yolo2_hip_ctx *c, int layer_idx, int frame, int8_t *out, size_t cap, int *geom)
{
    int rc = need_i8(c);
    if (rc) return rc;
    Y2I8 *s = c->i8;
    if (s->last_batch <= 0 || s->batch != s->last_batch) return fail(YOLO2_ERROR, "no int8 run to read (yolo2_hip_run_batch_int8)");
    if (layer_idx < -1 || layer_idx > 29) return fail(YOLO2_ERROR, "layer %d holds no int8 tensor (-1 = the quantised input, 0..29)", layer_idx);
    if (frame < 0 || frame >= s->last_batch) return fail(YOLO2_ERROR, "frame %d outside the last batch of %d", frame, s->last_batch);
    if (layer_idx < 1 && s->last_fused)
        return fail(YOLO2_ERROR, "layer %d was not written: the last int8 run was an images call, whose fused front kernel goes from the image bytes to "
                                 "layer 1 (option i8_no_front runs the frames route)", layer_idx);
    const Y2I8Tensor &t = layer_idx < 0 ? s->t_in : s->t[layer_idx];
    if (!t.d) return fail(YOLO2_ERROR, "layer %d holds no int8 tensor", layer_idx);
    if (geom) { geom[0] = t.C; geom[1] = t.H; geom[2] = t.W; geom[3] = t.q; }
    if (!out) return YOLO2_SUCCESS;
    const long n = (long)t.C * t.H * t.W;
    if (cap < (size_t)n) return fail(YOLO2_ERROR, "buffer of %zu elements is short of the tensor's %ld", cap, n);
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    HIP_TRY(hipDeviceSynchronize(), YOLO2_ERROR);
    Y2DevBuf<signed char> dense;
    if ((rc = dense.alloc(n))) return rc;
    hipLaunchKernelGGL(k_i8_unpack_nchw, dim3(blocks_for(n, 256)), dim3(256), 0, nullptr, (const signed char *)(t.d + (long)frame * t.H * t.W * t.cs),
                       dense.get(), t.C, t.cs, t.H * t.W, n);
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipMemcpy(out, dense.get(), (size_t)n, hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}

// ---------------------------------------------------------------------------- driver tier (yolo2_driver.hip holds the lock and has bound the device)

int y2_drv_conv_i8(uint64_t in, uint64_t out, uint64_t w, uint64_t bias, const int32_t *weight_q, int C, int N, int K, int W, int H, int batch,
                   int q_in, int q_out, int leaky, int out_float)
{
    const long per = (long)C * K * K;
    std::vector<int8_t> w_host((size_t)N * per);
    std::vector<int32_t> b_host(N);
    HIP_TRY(hipMemcpy(w_host.data(), (const void *)(uintptr_t)w, w_host.size(), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(b_host.data(), (const void *)(uintptr_t)bias, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost), YOLO2_DMA_ERROR);
    const int Np = round_up(N, tile_m(N)), Cp = round_up(C, kI8Granule), HW = H * W;
    std::vector<int> sh_host(Np, 0), bias_host(Np, 0);
    int rc = check_layer("yolo2_execute_conv_layer_int8", w_host.data(), b_host.data(), weight_q, N, per, q_in, q_out, out_float != 0, sh_host.data());
    if (rc) return rc;
    memcpy(bias_host.data(), b_host.data(), (size_t)N * sizeof(int));
    const long P = (long)batch * HW;
    const int ocs = round_up(N, kI8Granule);
    Y2DevBuf<signed char> xin, wpk, yout;
    Y2DevBuf<int> dbias, dsh;
    if ((rc = xin.alloc((size_t)P * Cp)) || (rc = wpk.alloc((size_t)K * K * (Cp / 32) * Np * 32)) || (rc = dbias.alloc(Np)) || (rc = dsh.alloc(Np)) ||
        (!out_float && (rc = yout.alloc((size_t)P * ocs))))
        return rc;
    HIP_TRY(hipMemcpy(dbias.get(), bias_host.data(), (size_t)Np * sizeof(int), hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    HIP_TRY(hipMemcpy(dsh.get(), sh_host.data(), (size_t)Np * sizeof(int), hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    hipLaunchKernelGGL(k_i8_pack_nchw, dim3(blocks_for(P * Cp, 256)), dim3(256), 0, nullptr, (const signed char *)(uintptr_t)in, xin.get(), C, Cp, HW,
                       P * Cp);
    launch_pack_weights((const signed char *)(uintptr_t)w, wpk.get(), N, C, K, Np, nullptr);
    ConvI8Args a;
    a.in = xin.get(); a.w = wpk.get(); a.bias = dbias.get(); a.sh = dsh.get();
    a.out = out_float ? (void *)(uintptr_t)out : (void *)yout.get();
    a.CC = Cp / 32; a.K = K; a.H = H; a.W = W; a.P = (int)P;
    a.N = N; a.Np = Np; a.ocs = ocs; a.leaky = leaky ? 1 : 0;
    launch_conv(a, out_float != 0, nullptr);
    if (!out_float) {
        const long n = P * N;
        hipLaunchKernelGGL(k_i8_unpack_nchw, dim3(blocks_for(n, 256)), dim3(256), 0, nullptr, (const signed char *)yout.get(),
                           (signed char *)(uintptr_t)out, N, ocs, HW, n);
    }
    HIP_TRY(hipGetLastError(), YOLO2_ERROR);
    HIP_TRY(hipStreamSynchronize(nullptr), YOLO2_ERROR);   // the scratch above is freed on return
    return YOLO2_SUCCESS;
}
