// y2_internal.hpp -- what the translation units of libyolo2_hip.so share (nothing here is part of the C ABI).
//
//   yolo2_hip.hip     errors, model tables (kNet: what the layers are; kWiring: how they are connected - "the wiring" below), context lifecycle, profiling, pre-processing, host-buffer streaming entries
//   yolo2_driver.hip  tier 1: the reference's accelerator-driver interface (linux_app/include/yolo2_accel_linux.h,
//                     dma_buffer_manager.h): device state, buffers, register file, per-layer calls
//   yolo2_int16.hip   the int16 path: weight loading / arithmetic-form proofs, launch planning, autotune, run_batch_int16
//   yolo2_fp16.hip    the fp16 MFMA path: weight packing, per-context launch table, run_batch_fp16
//   yolo2_fp32.hip    the exact fp32 path (tiled and one-thread-per-output)
//   yolo2_calib.hip   fp32 weights + calibration frames -> Q tables and int16 weights (statistics of the exact fp32 pass)
//   yolo2_int8.hip    the int8 pass on the i8 matrix cores: quantiser, loader and its proofs, run_batch_int8, the pass from a chunk of
//                     image bytes (k_i8_front_pix + layers 2..30), the single-layer call
//   yolo2_post.hip    region layer + boxes + NMS;   yolo2_multi.hip  frame sharding + the RCCL weight broadcast
//   yolo2_draw.hip    annotated frames: records + frames -> RGB24 with the reference's boxes and tags
//   yolo2_jpeg.hip    RGB24 frames in device memory -> the reference's JPEG streams
//   yolo2_loop.hip    the camera loop as one call: frames -> records and annotated frames from one upload (launches nothing itself)
//   yolo2_jpegdec.hip JPEG streams -> RGB24 in the chunk staging layout (probe, host doorway, decoder kernels) and the entries behind it
// Every non-template kernel is launched from exactly one of them (its kernels_*.hpp is included there only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/yolo2_hip.h"
#include "conv_common.hpp"
#include "layout.hpp"
#include "y2_mem.hpp"

// ---------------------------------------------------------------------------- errors (yolo2_hip.hip)

// stores the message for yolo2_hip_last_error() (thread-local) and returns `code`
int y2_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail y2_fail

#define HIP_TRY(expr, code)                                                                      \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(code, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)


// ---------------------------------------------------------------------------- options (yolo2_plan.hip)
//
// Every switch that steers kernel selection, lanes or planning lives here, ONE object per context: filled from the environment
// (YOLO2_<NAME>, upper case) once, when the context is created, and changed on a live context only through
// yolo2_hip_set_option(ctx, "<name>", "<value>").  Nothing on a planning or launch path calls getenv (round 3 read 26 variables at
// plan time, several of them per plan_conv call).  A lane inherits its parent's object.  README.md lists the names.
// Groups: (a) planning knobs a deployment may set (autotune, plan_file, plan_write, lanes, no_lanes, lane_priority, verbose);
// (b) A/B switches of kernel families (no_* / f16_*); (c) test hooks that force one kernel shape everywhere (force_*, f32_p).
struct Y2Options {
    // (a)
    int autotune = -1;            // -1: weight cache, then plan table, then timing; 0: static defaults, nothing timed; 1: always time
    std::string plan_file;        // replaces config/plan_gfx950.txt next to the library
    std::string plan_write;       // append every timed plan to this file (tools/make_plan.py)
    int lanes = 0;                // int16 lanes (0 = the default rule: 3 for batches 48..127, 2 from batch 16)
    bool no_lanes = false;
    std::string lane_split;       // diagnostic: "20,22,22"
    int lane_priority = 1;        // 0: lanes at default stream priority, lane 0 on the caller's stream (round-3 interim design)
    bool verbose = false;
    bool no_plan_cache = false;   // ignore a bound weight-side plan cache
    // (b)
    int splitk = -1;              // -1 tuned; 0 no K-split of either kind; 1 the lane-split kernel wherever legal
    int poolfuse = -1;            // 1: conv + pool fused wherever legal
    bool no_poolfuse = false, no_hiacc = false, no_ks = false, no_w16 = false, no_grp = false, grp16 = false, no_xcd_remap = false, splitk_no_pack = false,
         no_edge_tiles = false;   // (no_edge_tiles: raster tiles for the 3x3 form C / D launches, A/B - it changes no plan field)
    int f16_lanes = 2;
    bool f16_no_lanes = false, f16_no_mfma0 = false, f16_no_glds = false, f16_no_poolfuse = false, f16_no_halo = false, f16_no_persist = false,
         f16_persist_all = false, f16_ring_all = false, f16_no_ring = false, f16_no_c32 = false, f16_m16 = false, f16_w8 = false, f16_no_wide = false,
         f16_no_fuse1x1 = false, f16_no_rw = false, f16_no_rwb = false, f16_no_rwc = false, f16_ring256 = false, f16_ring_sq = false;
    bool i8_no_front = false;     // the int8 images entries letterbox into float frames and run the frames route (the reference route of
                                  // k_i8_front_pix's tests and report, as f16_no_mfma0 is for the fp16 entries)
    int jpegdec_split = 0;        // the GPU JPEG decoder's entropy stage with many lanes per segment: subsequence bytes, a multiple of 16 in
                                  // 16..4096 (0: one lane per segment, today's launches); read per call
    int stamp_layer = -1;
    int f16_skip = 0;             // DIAGNOSTIC (results wrong by construction): bit mask of fp16 launches left out of the table, to measure
                                  // what a launch costs INSIDE the two-lane step: 1 = 1x1 layers 5 and 9, 2 = layer 0, 4 = layers 2/4/6,
                                  // 8 = pools + reorg, 16 = the other 1x1 layers, 32 = the 13x13 3x3 layers
    // (c)
    int force_path = -1, force_p = 0, force_ks = 0, f32_p = 0;
    bool force_w16 = false, force_hiacc = false;

    static Y2Options from_env();
    // 0 = set, -1 = unknown name / bad value.  value NULL or "" restores the default.
    int set(const char *name, const char *value);
    // the settings that differ from the defaults, "name=value name=value" ("" if none): what bench.py discloses
    std::string describe() const;
    // switches that ask for a plan the committed table / the weight cache do not hold: those are bypassed
    bool steered() const { return splitk >= 0 || poolfuse >= 0 || no_poolfuse || no_w16 || no_hiacc || no_ks || no_grp || no_xcd_remap; }   // (grp16 keeps the plan sources: it changes no plan field)
};
const Y2Options &y2_process_options();   // from the environment, parsed once: the context-less driver tier and process-wide latches

// ---------------------------------------------------------------------------- launch plans as data (yolo2_plan.hip)

// One launch of a conv layer as the plan table / the weight cache store it:  B L S path P pad splitk pp w16 fuse hiacc ks
struct Y2PlanLine { int path, P, pad, splitk, pp, w16, fuse, hiacc, ks; };
typedef std::pair<int, std::pair<int, int>> Y2PlanKey;   // (B, (L, S))
// parses and range-checks one line (a line outside what the planner can produce is rejected); false: not a plan line
bool y2_plan_line_parse(const char *text, Y2PlanKey *key, Y2PlanLine *pl);
// the committed table (config/plan_gfx950.txt next to the library, or opt.plan_file): loaded once per file name
bool y2_plan_table_has_batch(const Y2Options &opt, int B);
bool y2_plan_table_lookup(const Y2Options &opt, int B, int L, int S, Y2PlanLine *out);

// The K-split-across-workgroups kernel's scratch rule on plain numbers (also exported: yolo2_hip_i16_plan_check):
// `splits` triples of 24 bytes per output item; cap = 0 (a context without scratch) refuses every split.
bool y2_ks_fits(int splits, int cg_out, int npix, size_t cap_bytes);
size_t y2_ks_bytes(int splits, int cg_out, int npix);

// The weight-side cache: one small text file beside a weight set, keyed by a hash of the blobs and Q tables,
// holding what loading and planning would otherwise recompute - the per-block bounds behind the arithmetic-form proofs (so
// k_weight_bound* is skipped), the forms and scale shifts derived from them (re-derived and compared at load: a mismatch drops the
// file) and the conv plan of every batch this weight set has been timed for (so the autotune is skipped and every process runs
// the same kernels).  A missing, stale or damaged file costs time, never correctness: hash and body checksum must both match.
struct Y2PlanCache {
    std::mutex mu;
    std::string path;
    uint64_t hash = 0;            // of the weight set currently loaded (0 = none yet)
    bool bounds_valid = false;    // the file matched this weight set and its bounds were used
    struct Bounds { int maxsum = 0, maxbias = 0; std::vector<int> sum_mb, bias_mb, abs_mb, form, scale; };
    Bounds bounds[YOLO2_N_CONV];
    std::map<Y2PlanKey, Y2PlanLine> lines;
    std::map<int, int> per_batch;
    bool dirty = false;
    // reads `path`; true iff header, hash and checksum match `want_hash` (then bounds / lines are filled)
    bool load(uint64_t want_hash, std::string *why);
    bool save();                   // temp file + rename; false (and nothing else) if the directory is not writable
};
uint64_t y2_hash_bytes(uint64_t seed, const void *data, size_t n);   // host side: Q tables, file body

// ---------------------------------------------------------------------------- model table (yolo2_hip.hip)

enum LType { L_CONV, L_MAX, L_ROUTE, L_REORG, L_REGION };
struct LayerDesc {
    LType type;
    int c, h, w, n, size, leaky;
};
// config/yolov2.cfg as parsed by the reference; the C host re-derives the same
// table from the .cfg file and checks it against this one before using the batched entry.
extern const LayerDesc kNet[32];

// ---------------------------------------------------------------------------- the wiring (yolo2_hip.hip)
//
// kNet says what every layer IS; this says how the layers are CONNECTED.  It is computed once, at compile time, from kNet, the stream
// lengths and the two [route] lines of config/yolov2.cfg, and it checks itself (static_assert: every reader's c, h, w are its source
// tensor's).  Every pass reads the graph from here: which tensor a layer reads, which outputs share the concat tensor and from
// which channel, which tensor has a second reader, which conv writes the region buffer, conv ordinals and stream offsets.
// A literal layer number may still name a MEASURED CHOICE about a layer (the fp16 kernel policy, the f16_skip masks, layer 0's fused
// front kernels); it may not restate a fact of the graph.
struct NetWire {
    int ord;               // conv ordinal, -1 otherwise
    long w_off, b_off;     // a conv's first element in the reference's weight / bias streams
    int n_route, route[4]; // a route layer's sources as the cfg lists them, absolute
    int src;               // the layer whose output tensor this layer reads (-1: the network input), routes resolved: a route of one
                           // source stands for that source, a route of several is the concat tensor and stands for itself
    int cat, ch_off;       // cat >= 0: the output lives in the concat tensor of route layer `cat`, from channel ch_off on (the cfg's order)
    int readers, reader;   // how many layers read the output (through routes), and the first of them (-1: none)
    bool to_region;        // the region layer reads it: the pass hands this output to the caller
    int C, H, W;           // shape of the tensor the output lives in (a member of the concat: the concat's)
};
struct NetWiring {
    NetWire layer[32];
    int conv_layer[YOLO2_N_CONV];   // ord -> layer
    int cat_conv, cat_feed;         // the concat's conv member, and the conv its reorg member reads: the two whose Qs the concat ties together
};
extern const NetWiring kWiring;
static constexpr const NetWire (&kWire)[32] = kWiring.layer;
static constexpr const int (&kConvLayer)[YOLO2_N_CONV] = kWiring.conv_layer;
// slot of an activation-Q table (slot 0: the network input, slot k + 1: the output of conv k) for the Q layer's output tensor carries:
// pools and the reorg keep their input's, the concat tensor carries its conv member's
static inline int y2_act_q_slot(int layer)
{
    while (layer >= 0 && kWire[layer].ord < 0) layer = kNet[layer].type == L_ROUTE ? kWiring.cat_conv : kWire[layer].src;
    return layer < 0 ? 0 : kWire[layer].ord + 1;
}

static inline unsigned blocks_for(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline long packed_weight_elems(int C, int N, int K)
{
    return (long)((N + y2::kTm - 1) / y2::kTm) * ((C + y2::kTn - 1) / y2::kTn) * K * K * 128;
}

// ---------------------------------------------------------------------------- launch plan of one conv launch (int16 / fp32 tiled)

constexpr int kMaxTileItems = 2048;  // 8 staging registers x 256 threads (k_conv_i16 NST <= 8)

struct ConvPlan {
    int C = 0, N = 0, K = 0, H = 0, W = 0, leaky = 0;
    int Qw = 0, Qa_in = 0, Qa_out = 0, Qb = 0;
    int path = 0;  // 0 = form A, 1 = form B (pre-shifted accumulator), 3 = form C (packed int16), 4 = form D (C, shift-free), 2 = 64-bit
    int P = 8;
    int mb_count = 0;          // output-channel blocks this launch covers (0 = all of the layer)
    int splitk_ok = 0;         // the loader proved the split-K bounds for these blocks (|t| < 2^29, sums < 2^30)
    int splitk = 0;            // small batches: S K-splits x 64/S pixels per wavefront, shuffle-combined (k_conv_i16_splitk); 0 or S
    int splitk_pp = 1;         // pixels per lane of the split-K kernel (2: two pixel tiles share the staged weight slices)
    int splitk_pack = 0;       // the lane-split kernel carries packed int16 triples (form D launches)
    size_t ks_cap = 0;         // bytes of the context's triple scratch: plan_conv refuses a split whose triples would not fit
    int ks = 0;                // single frames: K-split across workgroups (k_conv_i16_ks + k_ks_finalize); 0 or the number of splits
    int hiacc = 0;             // form D launches only: 1 = the kernel keeps one accumulator register per channel (no v_perm: MODE 5)
    int w16 = 0;               // 1: k_conv_i16_w16 - two wavefronts of 16 output channels each per workgroup instead of four of 8
    int grp = 1;               // 1x1 convs: channel groups per barrier (8 when it divides CGin and fits LDS staging)
    int pool_fused = 0;        // conv + leaky + 2x2 pool in one kernel (k_conv_i16_pool): 1 = pooled tensor only, 2 = + full tensor
    int lds_pad = 0;           // extra dynamic LDS requested only to cap workgroups per CU (autotuned):
                               // fewer co-resident workgroups finish sooner each, which shortens the
                               // idle tail of layers that are only a few workgroup-generations long
    dim3 grid;
    int lds_bytes = 0;
    y2::ConvArgs args;
};

// ---------------------------------------------------------------------------- the context

// An activation tensor: geometry, the address kernels and launch tables use, and - in the struct that allocated it - the owner.
// An alias (slots 24 and 27 of every family are the concat tensor) carries geometry and address only: y2_view_of.
struct Tensor {
    y2::ActGeom g;
    int2 *d = nullptr;
    Y2DevBuf<int2> own;
};

// Device buffers of one post-processing call in flight (yolo2_post.hip)
struct Y2PostBufs {
    int cap_frames = 0;
    size_t cap_dets = 0;
    Y2DevBuf<float> rows, rows2;
    Y2DevBuf<int> totals, counts;
    Y2DevBuf<uint8_t> geom;          // [cap_frames] letterbox-correction records (y2_post_geom_bytes() each)
    Y2DevBuf<yolo2_hip_det> dets;    // [cap_frames][cap]
};

// Staging for the host-buffer entries (run_frames / run_images): two buffer sets and three streams
// (upload, kernels, download), kept with the context and grown on demand so that a caller streaming
// chunk after chunk does not pay pinned-memory allocation per call.
struct PipeBufs {
    size_t host_in = 0, dev_in = 0;   // capacities in bytes (dev_in: raw image bytes, 0 for float frames)
    int batch = 0;
    Y2PinBuf<uint8_t> hin[2];
    Y2DevBuf<uint8_t> dbytes[2];
    Y2DevBuf<float> din[2];
    Y2PinBuf<int16_t> hout[2];
    Y2DevBuf<int16_t> dout[2];
    hipStream_t s_in = nullptr, s_run = nullptr, s_out = nullptr;
    hipEvent_t e_in[2] = {nullptr, nullptr}, e_run[2] = {nullptr, nullptr}, e_out[2] = {nullptr, nullptr};
    hipEvent_t e_lane[2][8] = {};      // images -> detections entry: lane i has finished its part of the chunk in buffer set b (created on demand)
    // the tail as a pipeline stage (yolo2_hip_run_images_u8_dets): per buffer set its device buffers and pinned host mirrors
    int post_batch = 0, post_cap = 0;
    Y2PostBufs post[2];
    Y2PinBuf<uint8_t> hgeom[2];
    Y2PinBuf<yolo2_hip_det> hdets[2];
    Y2PinBuf<int> hcounts[2];
    // the fp16 / split-fp16 images entries: fp32 region tensors [batch][425][13][13] per buffer set (device; pinned mirrors for the
    // entry that returns them)
    int regf_batch = 0;
    Y2DevBuf<float> dregf[2];
    Y2PinBuf<float> hregf[2];
    // the JPEG entries (yolo2_jpegdec.hip): per buffer set the chunk's blob (descriptors, tables, status words, streams) pinned and on the
    // device, and the pinned status mirror; the coefficient and plane buffers are touched by kernels of s_run only, so one of each
    size_t jpg_blob = 0, jpg_samples = 0, jpg_status = 0;
    Y2PinBuf<uint8_t> hjpg[2];
    Y2DevBuf<uint8_t> djpg[2];
    Y2PinBuf<int> hjstatus[2];
    Y2DevBuf<int16_t> jcoef;
    Y2DevBuf<uint8_t> jplanes;
};

// Staging of yolo2_hip_annotate_images_pix_host (yolo2_draw.hip): two buffer sets - pinned and device staging for a chunk's table,
// draw items and frame bytes, device and pinned RGB24 output - and three streams, grown on demand and kept with the context.
struct Y2AnnoBufs {
    size_t cap_in = 0, cap_out = 0;
    Y2PinBuf<uint8_t> hin[2], hout[2];
    Y2DevBuf<uint8_t> din[2], dout[2];
    hipStream_t s_in = nullptr, s_run = nullptr, s_out = nullptr;
    hipEvent_t e_in[2] = {nullptr, nullptr}, e_run[2] = {nullptr, nullptr}, e_out[2] = {nullptr, nullptr};
};

// What yolo2_hip_annotate_images_pix_jpeg_host (yolo2_draw.hip) keeps beside Y2AnnoBufs' upload side and streams: the painted RGB24
// frames and the encoder's work area (touched by kernels of one stream only, so one of each), two sets of packed device and pinned
// output with the pinned per-frame sizes, grown on demand.
struct Y2JpegBufs {
    size_t cap_rgb = 0, cap_work = 0, cap_out = 0, cap_frames = 0;
    Y2DevBuf<uint8_t> rgb, work, dout[2];
    Y2PinBuf<uint8_t> hout[2];
    Y2PinBuf<unsigned long long> hsizes[2];
    hipEvent_t e_sizes[2] = {nullptr, nullptr};
};

// What the loop entry (yolo2_loop.hip) keeps beside PipeBufs and the two above: the draw list k_draw_items makes on the device - the
// complete painter table (header, frames, cap items per frame) and the per-frame {items, unprintable records}, each written and read
// on the download stream only, so one of each, with two pinned mirrors of the latter - and the call's label table.
struct Y2LoopBufs {
    size_t cap_table = 0, cap_labels = 0;
    int cap_frames = 0;
    Y2DevBuf<uint8_t> table, labels;
    Y2DevBuf<int> info;
    Y2PinBuf<int> hinfo[2];
};

struct F16Plan;   // yolo2_fp16.hip: the per-context launch table of the fp16 path
struct Y2I8;      // yolo2_int8.hip: packed int8 weights, Q tables and activation tensors of the int8 pass

struct yolo2_hip_ctx {
    PipeBufs pipe;
    Y2AnnoBufs anno;
    Y2JpegBufs jpeg;
    Y2LoopBufs loop;
    yolo2_hip_loop_info_t loop_info = {};   // of the last loop call (yolo2_hip_loop_last_info)
    double jpeg_dec_info[8] = {};           // of the last JPEG call (yolo2_hip_jpeg_last_info)
    double jpeg_split_info[8] = {};         // of the last JPEG call (yolo2_hip_jpeg_split_info): all zero without option jpegdec_split
    int device = 0;
    Y2Options opt;                     // parsed once at creation (environment), changed only by yolo2_hip_set_option; lanes copy it
    std::shared_ptr<Y2PlanCache> plan_cache;   // weight-side cache bound by yolo2_hip_set_plan_cache (lanes share the parent's)
    bool weights_loaded = false;
    // Weight buffers are an owner plus the view every user reads: the context that allocated a buffer fills both, a lane or the split
    // twin fills only the view of what it borrows from its parent (which outlives it: yolo2_hip_destroy, and every reload destroys
    // the borrowers before it replaces a buffer).
    short *wpk = nullptr;      // all layers, packed
    short *bias_pk = nullptr;  // all layers, padded to 32
    Y2DevBuf<short> wpk_own, bias_pk_own;
    long wpk_off[YOLO2_N_CONV], bias_off[YOLO2_N_CONV];
    int maxsum[YOLO2_N_CONV], maxbias[YOLO2_N_CONV];
    std::vector<int> weight_q, bias_q, act_q;
    ConvPlan plan[32];                 // per conv layer: the launch covering most output-channel blocks
    std::vector<ConvPlan> extra[32];   // further launches for blocks that need another arithmetic form
    std::vector<int> maxsum_mb[YOLO2_N_CONV], maxbias_mb[YOLO2_N_CONV], maxabs_mb[YOLO2_N_CONV];
    std::vector<signed char> wscale_mb[YOLO2_N_CONV];   // log2 of the factor each block's packed weights currently carry (form D)
    std::vector<signed char> form_mb[YOLO2_N_CONV];     // arithmetic form resolve_q chose per block of 32 output channels
    int *mb_lists = nullptr;           // device: block index lists of all split layers
    Y2DevBuf<int> mb_lists_own;
    int plan_source = 0;               // how set_batch planned the conv launches: 1 plan table, 2 timed (autotune), 3 static defaults, 4 forced, 5 weight cache
    int *ks_trip = nullptr;            // device scratch of the K-split-across-workgroups kernel (triples of every split): sized from the accepted plans
    Y2DevBuf<int> ks_trip_own;
    size_t ks_trip_bytes = 0;
    // Lanes: a batch is run as part-batches on internal streams (forked from / joined to the
    // caller's stream with events).  Every layer is then several concurrent launches, and the idle tail of
    // one (a layer is only a few workgroup-generations long at batch 64) is filled by the others.
    // A lane is a child context that shares the parent's weights.
    std::vector<yolo2_hip_ctx *> lanes;
    std::vector<int> lane_first;       // first frame of each lane within the batch
    std::vector<yolo2_hip_ctx *> f16_lanes;   // fp16 path: two half-batch lanes (share wh / biasf / w0f)
    bool is_lane = false, laned = false;
    hipStream_t lane_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool fuse_pool[32] = {false};      // conv layer i stores the pooled tensor of layer i+1 itself (k_conv_i16_pool)
    ConvPlan fplan[32];                // the fused launches of those layers (plan / extra keep the unfused ones)
    std::vector<ConvPlan> fextra[32];
    int path_counts[YOLO2_N_CONV][5];
    int reorg_shift = 0, final_q = 0;
    int batch = 0;
    Tensor t_in, t_out[32], t_cat;
    // ---- fp16 MFMA path
    struct HalfGeom {
        int C = 0, Cp = 0, H = 0, W = 0, Wp = 0, PL = 0, B = 0;
        size_t items = 0;
    };
    struct HalfTensor : HalfGeom {
        _Float16 *d = nullptr;
        Y2DevBuf<_Float16> own;
    };
    bool f16_loaded = false;
    // split-fp16 ("fp32tol") mode: a twin context that runs the fp16 launch table on items of three parts [hi | lo | hi] with
    // weights packed [w_hi | w_hi | w_lo] (kernels_f16.hpp, SPLIT instantiations).  The twin owns its packed weights (wh / biasf), its
    // tensors, table and lanes; it borrows the fp32 blobs and w0f from this context (views without owners).
    bool split = false;                // this context IS such a twin (or a lane of one)
    yolo2_hip_ctx *tol = nullptr;      // the parent's twin, made at the first yolo2_hip_run_batch_f32tol
    _Float16 *wh = nullptr;
    float *biasf = nullptr;
    float *w0f = nullptr;  // layer 0: [27][32] fp32 weights + [32] bias for the fused conv0+pool kernel
    float *wf32 = nullptr, *bf32 = nullptr;   // the fp32 blobs as loaded (reference stream order), for the exact fp32 pass
    Y2DevBuf<_Float16> wh_own;
    Y2DevBuf<float> biasf_own, w0f_own, wf32_own, bf32_own;
    F16Plan *f16_plan = nullptr;              // launch table of the fp16 pass (built once per (weights, batch); owned)
    std::string images_l0[2];                 // what the last fp16 (0) / split (1) images call ran for layers 0+1 (yolo2_hip_images_layer0_kernel)
    std::string images_front_i8;              // what the last int8 images call ran up to layer 1 (yolo2_hip_images_front_kernel_int8)
    // ---- tiled exact fp32 path (kernels_f32.hpp): packed weights [mb][cg][tap][32][4] floats, items of 4 floats
    float *wpkf = nullptr, *biasf32_pk = nullptr;
    Y2DevBuf<float> wpkf_own, biasf32_pk_own;
    long wpkf_off[YOLO2_N_CONV], biasf32_off[YOLO2_N_CONV];
    struct FTensor {
        y2::ActGeom g;
        float4 *d = nullptr;
        Y2DevBuf<float4> own;
    };
    int f32_batch = 0;
    FTensor f_in, f_out[32], f_cat;
    ConvPlan fp32_plan[32];
    // ---- calibration (yolo2_calib.hip): abs-max statistics of the exact fp32 pass's tensors, accumulated over yolo2_hip_calib_frames
    // calls.  Pairs of uint32 {max |x| as fp32 bits, saturating count of non-finite values}; allocated at the first calibration call.
    Y2DevBuf<unsigned> calib_stats;
    long calib_frames_seen = 0;
    Y2I8 *i8 = nullptr;                // the int8 pass (made by yolo2_hip_load_weights_int8; owned: y2_i8_free)
    long wh_off[YOLO2_N_CONV], biasf_off[YOLO2_N_CONV];
    int f16_batch = 0;
    int f16_last_batch = 0;            // batch of the last yolo2_hip_run_batch_fp16 on this context (yolo2_hip_debug_f16_tensor)
    bool f16_last_laned = false;       // ... and whether it ran as lanes (f16_lanes hold the tensors then)
    HalfTensor h_in, h_out[32], h_cat;
    // per-layer device timing: a ring of event sets, one per profiled run (hipEvents on the
    // stream the kernels are launched on); the analogue of yolo2_inference.c:75-142
    static constexpr int kProfSlots = 32;
    bool prof = false;
    hipEvent_t ev[kProfSlots][33];
    bool ev_made = false;
    long prof_runs = 0;
};

// ---------------------------------------------------------------------------- helpers that cross translation units

// yolo2_hip.hip
// drops the tensors of one family (owners and views) and its batch: c->t_* / batch, c->h_* / f16_batch, c->f_* / f32_batch
template <typename TensorT>
void y2_free_tensors(TensorT &in, TensorT (&out)[32], TensorT &cat, int &batch)
{
    for (TensorT *t : {&in, &cat}) { t->own.reset(); t->d = nullptr; }
    for (TensorT &t : out) { t.own.reset(); t.d = nullptr; }
    batch = 0;
}
void y2_free_activations(yolo2_hip_ctx *c);       // the int16 family and its K-split scratch
void y2_destroy_lanes(yolo2_hip_ctx *c);
// Streams of the lanes (yolo2_hip.hip): created at the device's HIGHEST stream priority.  HIP multiplexes the streams of a process
// onto a few hardware queues PER PRIORITY LEVEL (4 by default); at the default priority the lanes share that pool with every other
// stream of the process - the streaming entries' copy streams, torch's and RCCL's internal streams - and two lanes that land on one
// queue run one after the other (measured: -5 % under torch.distributed, -10 % in the streaming entry).  At their own level the
// lanes have a pool to themselves.  own_stream_for_lane0 = false (YOLO2_LANE_PRIORITY=0, the round-3 interim design): default
// priority, lane 0 runs on the caller's stream.
int y2_lane_stream_create(hipStream_t *s);
bool y2_lane0_own_stream();
int y2_ensure_prof_events(yolo2_hip_ctx *c);

// allocates `count` elements into `own` and points the view `d` at them (nullptr if the allocation fails)
template <typename T>
int y2_alloc_owned(Y2DevBuf<T> &own, T *&d, size_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE())
{
    d = nullptr;
    const int rc = own.alloc(count, file, line);
    d = own.get();
    return rc;
}
// `v` becomes an alias of `of`: its geometry and address, owning nothing
template <typename TensorT>
void y2_view_of(TensorT &v, const TensorT &of)
{
    v.own.reset();
    v.g = of.g;
    v.d = of.d;
}
inline void y2_view_of(yolo2_hip_ctx::HalfTensor &v, const yolo2_hip_ctx::HalfTensor &of)
{
    v.own.reset();
    static_cast<yolo2_hip_ctx::HalfGeom &>(v) = of;
    v.d = of.d;
}
// the item tensor (Tensor, FTensor) of a [C][H][W] map for B frames, zero-filled: the zeros ARE the conv padding (fp32: +0.0f, also
// the 4th lane of the input)
template <typename TensorT>
int y2_alloc_items(TensorT &t, int C, int H, int W, int B)
{
    t.g = y2::make_geom(C, H, W, B);
    const int rc = y2_alloc_owned(t.own, t.d, (size_t)t.g.items);
    if (rc) return rc;
    HIP_TRY(hipMemset(t.d, 0, (size_t)t.g.items * sizeof(*t.d)), YOLO2_DMA_ERROR);
    return YOLO2_SUCCESS;
}
// The tensors of one family as the wiring places them: every conv and pool layer owns a tensor, except that the members of a concat
// (and its route layer's slot) are views of `cat`, so out[] is indexed by NetWire::src.  alloc(tensor, layer) allocates for that
// layer's NetWire shape; a family may leave a layer without a tensor (d == nullptr).
template <typename TensorT, typename Alloc>
int y2_alloc_tensors(TensorT (&out)[32], TensorT &cat, Alloc alloc)
{
    for (int i = 0; i < 32; ++i) {
        const NetWire &w = kWire[i];
        int rc = YOLO2_SUCCESS;
        if (w.cat >= 0) {
            if (!cat.d && (rc = alloc(cat, w.cat))) return rc;
            y2_view_of(out[i], cat);
        } else if ((kNet[i].type == L_CONV || kNet[i].type == L_MAX) && (rc = alloc(out[i], i))) return rc;
    }
    return YOLO2_SUCCESS;
}
// what conv layer i of an item-layout family (int16, tiled fp32) reads and writes, and the first item of its output: a member of the
// concat starts at its channel group there
template <typename TensorT>
struct Y2ConvIO { const TensorT *tin, *tout; long out_base; };
template <typename TensorT>
Y2ConvIO<TensorT> y2_conv_io(int i, const TensorT &in, const TensorT (&out)[32])
{
    const NetWire &w = kWire[i];
    return {w.src < 0 ? &in : &out[w.src], &out[i], y2::kLead + (long)(w.ch_off / 4) * out[i].g.cg_stride};
}
// frames on the host -> device, `run(frames_dev, region_dev)` on the null stream, the region tensor (elements of R) back: the four
// yolo2_hip_run_batch_*_host entries
template <typename R, typename Run>
int y2_run_batch_host(yolo2_hip_ctx *c, const float *frames, int batch, R *region, Run run)
{
    if (!c || !frames || !region) return fail(YOLO2_ERROR, "null argument");
    HIP_TRY(hipSetDevice(c->device), YOLO2_INIT_ERROR);
    Y2DevBuf<float> fd;
    Y2DevBuf<R> rd;
    int rc;
    if ((rc = fd.alloc((size_t)batch * YOLO2_FRAME_ELEMS)) || (rc = rd.alloc((size_t)batch * YOLO2_REGION_ELEMS))) return rc;
    HIP_TRY(hipMemcpy(fd.get(), frames, (size_t)batch * YOLO2_FRAME_ELEMS * sizeof(float), hipMemcpyHostToDevice), YOLO2_DMA_ERROR);
    rc = run((uint64_t)(uintptr_t)fd.get(), (uint64_t)(uintptr_t)rd.get());
    if (rc == YOLO2_SUCCESS) {
        const hipError_t e = hipMemcpy(region, rd.get(), (size_t)batch * YOLO2_REGION_ELEMS * sizeof(R), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(YOLO2_DMA_ERROR, "D2H of region tensor failed: %s", hipGetErrorString(e));
    }
    return rc;
}

// yolo2_fp16.hip
void y2_f16_plan_free(yolo2_hip_ctx *c);
// The fp16 images entries (yolo2_hip.hip).  y2_f16_images_ctx: the context whose pass they run - c itself (split 0) or its split twin
// (split 1, made here) - or YOLO2_ERROR without fp32 weights.  y2_f16_images_fused: that pass has the layer-0 step from bytes (not under
// f16_no_mfma0: the entries then letterbox into frames and run the frame path).  y2_f16_run_images: the pass on a chunk of `batch`
// frames whose staging buffer (LetterboxItem table + images) is at lb, enqueued on st; y2_f16_images_kernel names its layer-0 kernel.
// kind: what the chunk's images are (Y2PixKind below) - interleaved bytes, packed YUYV 4:2:2, planar 4:2:0 or packed BGR24 / RGBA32 / BGRA32 frames.
int y2_f16_images_ctx(yolo2_hip_ctx *c, int split, yolo2_hip_ctx **run);
bool y2_f16_images_fused(const yolo2_hip_ctx *run);
int y2_f16_run_images(yolo2_hip_ctx *run, const uint8_t *lb, int kind, int batch, float *region_dev, hipStream_t st);
const char *y2_f16_images_kernel(const yolo2_hip_ctx *run, int kind);

// The per-layer driver calls' device work (yolo2_driver.hip validates, latches the register file, takes the lock, binds the
// device, and synchronises with the reference's timeout semantics afterwards; these only enqueue on the null stream).
// yolo2_int16.hip:
int y2_drv_conv_i16(const short *in, short *out, const short *w, const short *beta, int ifm, int ofm, int ksize, int kstride,
                    int iw, int ih, int ow, int oh, int pad, int is_nl, int qw, int qa_in, int qa_out, int qb, int *path_out);
void y2_drv_pool_i16(const short *in, short *out, int channels, int ksize, int kstride, int iw, int ih, int ow, int oh);
void y2_drv_release_i16(void);   // frees the grow-only scratch of y2_drv_conv_i16 (yolo2_accel_cleanup)
// yolo2_fp32.hip:
void y2_drv_conv_f32(const float *in, float *out, const float *w, const float *beta, int ifm, int ofm, int ksize, int kstride, int iw,
                     int ih, int ow, int oh, int pad, int is_nl);

// yolo2_int8.hip: the driver tier's int8 conv (buffers in natural dense order; synchronises the null stream), and c->i8's end
int y2_drv_conv_i8(uint64_t in, uint64_t out, uint64_t w, uint64_t bias, const int32_t *weight_q, int C, int N, int K, int W, int H, int batch,
                   int q_in, int q_out, int leaky, int out_float);
void y2_i8_free(yolo2_hip_ctx *c);
// The int8 images entries (yolo2_hip.hip), the siblings of y2_f16_images_fused / y2_f16_run_images / y2_f16_images_kernel:
// y2_i8_images_fused is false under i8_no_front (the entries then letterbox into frames and call yolo2_hip_run_batch_int8);
// y2_i8_run_images runs k_i8_front_pix on the chunk's staging buffer at lb into layer 1's tensor and layers 2..30 behind it, on st.
bool y2_i8_loaded(const yolo2_hip_ctx *c);
bool y2_i8_images_fused(const yolo2_hip_ctx *c);
int y2_i8_run_images(yolo2_hip_ctx *c, const uint8_t *lb, int kind, int batch, float *region_dev, hipStream_t st);
const char *y2_i8_front_kernel(int kind);

// yolo2_draw.hip: the streams, events and buffers of c->anno (yolo2_hip_destroy)
void y2_anno_free(yolo2_hip_ctx *c);
void y2_anno_jpeg_free(yolo2_hip_ctx *c);   // c->jpeg
int y2_anno_ensure(yolo2_hip_ctx *c, size_t cap_in, size_t cap_out);
int y2_anno_jpeg_ensure(yolo2_hip_ctx *c, size_t cap_rgb, size_t cap_work, size_t cap_out, size_t frames);
// ... and the device draw list of the loop entry (yolo2_loop.hip drives it; k_draw_items and the painter are launched here).
// geom: the painter's table as the host knows it before the records exist (y2_loop_geom_bytes(nf) bytes; returns the most strips of a
// frame).  _enqueue_items: k_draw_items on st from the records / counts of one tail, then the D2H of the per-frame
// {items, unprintable} into c->loop.hinfo[b].  _enqueue_paint: the painter of out_format (k_annotate_batch, _bgr, _nv12, _i420; the JPEG
// route paints RGB24) over the table _enqueue_items left.  out_format (YOLO2_LOOP_OUT_*) also decides what _fill_geom returns: the
// grid of the 4:2:0 painters counts patches, not flat strips (AnnoFrame::strips itself stays the flat count).
void y2_loop_free(yolo2_hip_ctx *c);
size_t y2_loop_geom_bytes(int nf);
int y2_loop_fill_geom(uint8_t *geom, int nf, const int *widths, const int *heights, int ch, const size_t *src_off, const size_t *out_off, int out_format);
int y2_loop_ensure(yolo2_hip_ctx *c, int frames, int cap, const char *const *labels, int n_labels);
int y2_loop_enqueue_items(yolo2_hip_ctx *c, int b, int nf, int cap, float thresh, const char *const *labels, int n_labels, const uint8_t *geom_dev,
                          const yolo2_hip_det *dets_dev, const int *counts_dev, hipStream_t st);
int y2_loop_enqueue_paint(yolo2_hip_ctx *c, int nf, int max_strips, const uint8_t *src_base, uint8_t *out_base, int out_format, hipStream_t st);

// yolo2_hip.hip: what the images entries and the loop entry share - the letterbox rule, the chunk letterbox launch, PipeBufs' growth
// (need_hout: the pinned region mirrors; _post: the tail's buffers; _regf: the fp32 region tensors) and the threaded staging copy
namespace y2 { struct LetterboxArgs; }
// The pixel formats of the _pix entries, one descriptor each: everything the host code needs to know about a format.
//   ch      what LetterboxArgs::ch / AnnoFrame::ch carry: bytes per pixel for interleaved bytes (1, 3) and YUYV (2); for the planar
//           4:2:0 formats, which have no whole number of bytes per pixel, and for packed BGR24 / RGBA32 / BGRA32, whose byte counts
//           3 and 4 would not tell them from RGB24, a code that only their own fetch looks at
//   kind    which kernels read it (the letterbox, layer-0, int8-front and painter instantiations)
//   frame_bytes(w, h)   size of a frame; sizes staging, offsets and geometry everywhere
//   even_w / even_h     the parity rule; align: the address alignment the single-image entries ask for
enum Y2PixKind { Y2_KIND_BYTES = 0, Y2_KIND_YUYV, Y2_KIND_NV12, Y2_KIND_I420, Y2_KIND_BGR24, Y2_KIND_RGBA32, Y2_KIND_BGRA32, Y2_KIND_COUNT };
struct Y2PixDesc {
    int pixfmt;
    const char *name;
    int ch;
    Y2PixKind kind;
    int bits;   // per pixel
    bool even_w, even_h;
    unsigned align;
    size_t frame_bytes(int w, int h) const { return (size_t)w * h * bits / 8; }
};
const Y2PixDesc *y2_pix_desc(int pixfmt, const char *who);   // by YOLO2_PIX_* fourcc; nullptr and "[who: ]unknown pixel format" otherwise
const Y2PixDesc *y2_pix_desc_ch(int ch);                     // by its ch; nullptr for a ch no format has
inline size_t y2_frame_bytes(int w, int h, int ch)
{
    const Y2PixDesc *d = y2_pix_desc_ch(ch);
    return d ? d->frame_bytes(w, h) : (size_t)w * h * ch;
}
inline int y2_ch_kind(int ch)
{
    const Y2PixDesc *d = y2_pix_desc_ch(ch);
    return d ? d->kind : Y2_KIND_BYTES;
}
// the parity rule of a frame: YOLO2_ERROR "who: NAME frames have an even width, not W" (... height ...)
int y2_pix_check_parity(const Y2PixDesc &d, int w, int h, const char *who, int frame);
// channels: a Y2PixDesc::ch.  pix: called from a _pix entry; the u8 entries, whose callers pass a channel count, take 1 and 3 only.
int y2_letterbox_args(int w, int h, int channels, int net_w, int net_h, y2::LetterboxArgs &a, bool pix);
const char *y2_letterbox_batch_kernel(int kind);
void y2_launch_letterbox_batch(int kind, const uint8_t *dbytes, float *din, int batch, hipStream_t st);
int y2_pipe_ensure(PipeBufs &p, size_t host_in, size_t dev_in, int batch, bool need_hout);
int y2_pipe_ensure_post(yolo2_hip_ctx *c, int batch, int cap);
int y2_pipe_ensure_regf(PipeBufs &p, int batch, bool need_host);
void y2_stage_images(uint8_t *dst, const uint8_t *const *images, const size_t *offs, const size_t *bytes, int nf);
// the network of the chunk in buffer set b (staged, its upload waited for on s_run), enqueued: int16 into dout[b], with the events whoever
// needs the whole region tensor waits for (the lanes are not joined); fp16 / split into dregf[b], e_run[b] recorded behind it
int y2_pipe_enqueue_i16(yolo2_hip_ctx *c, int b, int kind, int batch, int *q, std::vector<hipEvent_t> *done);
int y2_pipe_enqueue_f16(yolo2_hip_ctx *c, yolo2_hip_ctx *run, bool fused, int b, int kind, int batch);

// yolo2_calib.hip: one exact fp32 pass over `batch` device frames + the abs-max reductions, accumulated into c->calib_stats; `counted`
// of the frames are new ones (the images entry pads a short last chunk by repeating its last image).  Synchronises st.
int y2_calib_frames(yolo2_hip_ctx *c, uint64_t frames_dev, int batch, int counted, hipStream_t st);

// yolo2_post.hip: the tail (region + boxes + NMS + record compaction) as a stage of a pipeline - caller-owned buffers, enqueue only.
int y2_post_alloc(int device, int batch, int cap, Y2PostBufs *b);
size_t y2_post_geom_bytes(void);
int y2_post_fill_geom(void *geom_host, const int *im_w, const int *im_h, int n);   // host side: correct_region_boxes' per-frame constants
// region tensor [batch][425][13][13] int16 on `device` -> b->dets / b->counts (cap records per frame; best_only: one per detection);
// b->geom must hold the frames' records (copied on `st` in front of this call).  Enqueues on st, returns without synchronising.
// app_tail: the camera loop's tail (linux_app/src/yolo2_postprocess.c, YOLO2_DETS_APP_TAIL) instead of the src/core one.
int y2_post_enqueue_int16(int device, const int16_t *region_dev, int batch, int final_q, float thresh, float nms, int cap, int best_only,
                          int app_tail, Y2PostBufs *b, hipStream_t st);
// the same on an fp32 region tensor (the fp16 / split / fp32 passes; yolo2_hip_postprocess_f32 is this plus its synchronous copies).
// proc_dev (optional): the activated region tensor; final_rows (optional): the rows the records were compacted from.
int y2_post_enqueue_f32(const float *region_dev, int batch, float thresh, float nms, int cap, int best_only, int app_tail, Y2PostBufs *b,
                        hipStream_t st, float *proc_dev = nullptr, float **final_rows = nullptr);

