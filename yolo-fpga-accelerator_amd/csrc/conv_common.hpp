// conv_common.hpp -- what the int16 and the exact-fp32 conv kernels share: launch arguments, pixel-index arithmetic,
// the XCD-aware workgroup numbering, and the two templated layout kernels.  Header-only device code (inline / templates),
// safe to include from several translation units; every non-template __global__ kernel lives in exactly one kernels_*.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "layout.hpp"

namespace y2 {

typedef short short2_t __attribute__((ext_vector_type(2)));

struct ConvArgs {
    int B, H, W, Wp, PL;       // geometry shared by input and output ('same' conv, stride 1)
    int CGin;                  // input channel groups
    int CGout;                 // output channel groups that exist in the destination tensor
    int npix;                  // B*H*W
    long in_cg_stride;         // items
    long out_cg_stride;        // items
    long out_base;             // item offset of output group 0 (concat placement), incl. lead
    int shift, round;          // fast path: 0 <= shift <= 30, round = shift ? 1<<(shift-1) : 0
    int sh_right, sh_left;     // exact path: direction flags, magnitude = shift
    int bs_right, bs_left, bs_mag;  // bias shift (exact path computes it itself)
    int leaky;
    int lt_max;                // LDS tile capacity in items
    int xcd_remap;             // 0 = launch order; 1 + log2(Xm): XCDs as an (8/Xm) x Xm grid over (tiles, blocks)
    const int *mb_list;        // optional: blockIdx.y -> output-channel block (a layer whose blocks need
                               // different arithmetic forms is launched once per form); nullptr = identity
    // conv + leaky + 2x2/2 max pool fused (k_conv_i16_pool): geometry of the pooled destination tensor
    int nwin;                  // B * (H/2) * (W/2) pool windows
    int oWp, oPL;              // row pitch / plane size of the pooled tensor (items)
    long pool_cg_stride;       // items between channel groups of the pooled tensor
    long pool_base;            // item offset of its channel group 0, incl. lead
    // division by H*W, W (and, fused pool, by (H/2)*(W/2), W/2) as multiply-high + shift: layout.hpp fast_div, set by set_conv_div
    unsigned mHW, sHW, mW, sW, mOHW, sOHW, mOW, sOW;
    // K-split across workgroups (k_conv_i16_ks, small batches): grid.y = blocks x ks_S; split z runs channel groups [z ks_Q, (z + 1) ks_Q)
    // and leaves the clamp-affine triples of its sub-chains in ks_trip[z][channel item][pixel][2 pairs][a, l, h]
    int ks_S, ks_Q, ks_mb;     // splits, groups per split, blocks in this launch (grid.y / ks_S)
    int *ks_trip;
    // edge-class pixel tiles (k_conv_i16<3, 1, 3|4, NST, 1, true>; set by edge_tiles_plan, see there)
    int edge;                  // 1: grid.x counts edge-class tiles instead of raster tiles
    int e_nt, e_nb;            // tiles in all, band tiles among them
    int e_band[4];             // cumulative full-tile counts of the band classes: top, + bottom, + left, + right
    int e_int;                 // full interior tiles (the mixed tiles follow them)
    int e_n[5];                // pixels per class: top, bottom, left, right, interior
    int e_rem[6];              // cumulative class remainders n % 64: the mixed pixels of class c are [e_rem[c], e_rem[c + 1])
    unsigned mH2, sH2, mW2, sW2, mI2, sI2;   // division by H - 2, W - 2, (H - 2)(W - 2)
};

inline void set_conv_div(ConvArgs &a)
{
    auto one = [](unsigned d, unsigned &m, unsigned &s) { if (d < 2) { m = 0; s = 32; } else fast_div_magic(d, m, s); };   // s = 32: divisor 1
    one((unsigned)(a.H * a.W), a.mHW, a.sHW);
    one((unsigned)a.W, a.mW, a.sW);
    one((unsigned)((a.H / 2) * (a.W / 2)), a.mOHW, a.sOHW);
    one((unsigned)(a.W / 2), a.mOW, a.sOW);
}
__device__ __forceinline__ int div_c(int n, unsigned m, unsigned s) { return s >= 32 ? n : (int)fast_div((unsigned)n, m, s); }

// core_compute.cpp:191-197: x<0 ? x/10 (C division, toward zero) : x.  For u in [1,32768]
// floor(u/10) == (u*52429)>>19 (checked exhaustively in tests/test_host_logic.py).
__device__ __forceinline__ int leaky_i16(int v)
{
    const unsigned u = (unsigned)(-v);
    const int q = (int)((u * 52429u) >> 19);
    return v < 0 ? -q : v;
}

__device__ __forceinline__ int clamp16(int v) { return min(max(v, -32768), 32767); }

__device__ __forceinline__ long shift64(long v, int right, int left, int mag, long round)
{
    if (right) return (v + round) >> mag;
    if (left) return (long)((unsigned long)v << mag);
    return v;
}

// Darknet's legacy reorg (stride 2) as the reference runs it (yolo2_model.cpp:112-129): out[i + 26*(j + 416*k)] = x[(2i + k%2) + 52*(2j + k/2)]
// over the flat tensors.  From the flat output index o in [256][13][13]: the element (sc, sy, sx) of the logical [64][26][26] source.
struct ReorgSrc { int sc, sy, sx; };
__device__ __forceinline__ ReorgSrc reorg_src(int o)
{
    const int k = o / (26 * 416), rem = o - k * (26 * 416), j = rem / 26, i = rem - j * 26;
    const int sidx = (2 * i + (k & 1)) + 52 * (2 * j + (k >> 1));
    const int sc = sidx / 676, sr = sidx - sc * 676, sy = sr / 26;
    return {sc, sy, sr - sy * 26};
}

// Pixel index q (raster over b, y, x of real pixels) -> flat item offset inside a channel group.
__device__ __forceinline__ int flat_of(const ConvArgs &a, int q)
{
    const int b = div_c(q, a.mHW, a.sHW);
    const int r = q - b * (a.H * a.W);
    const int y = div_c(r, a.mW, a.sW);
    const int x = r - y * a.W;
    return b * a.PL + (y + 1) * a.Wp + x;
}

// ---- edge-class pixel tiles (3x3 'same' convs, H, W >= 3) ---------------------------------------------------------------------
//
// A tap outside the image reads a stored zero and its step leaves the accumulator as it was (sat16(acc + 0) = acc in every form),
// but a raster tile's 64 pixels span several rows, so no tap is out of the image for all of them.  Edge-class tiles group the real
// pixels by the set of taps that can be in the image:
//   top row (corners included, taps of rows 0, +1), bottom row (rows -1, 0), left column of rows 1 .. H-2 (columns 0, +1),
//   right column of rows 1 .. H-2 (columns -1, 0): 6 taps each; interior: 9 taps.
// Each class is ordered (b, y, x); its full 64-pixel tiles run only the class's taps.  The remainders of all five classes (< 64
// each) are concatenated into "mixed" tiles that run all 9.  Grid order: the band tiles are interleaved evenly among interior +
// mixed tiles (Bresenham), so that every XCD's contiguous tile range and every CU get the same share of 6-tap work.
// Host and device share these functions: the host partition check (yolo2_hip_i16_edge_map) runs exactly the kernel's decode.
enum { kEdgeTop = 0, kEdgeBottom = 1, kEdgeLeft = 2, kEdgeRight = 3, kEdgeInterior = 4, kEdgeMixed = 5 };

// taps (i, j) = (row 0..2, column 0..2) as bit 3i + j
__host__ __device__ constexpr int edge_class_mask(int cls)
{
    return cls == kEdgeTop ? 0x1f8 : cls == kEdgeBottom ? 0x03f : cls == kEdgeLeft ? 0x1b6 : cls == kEdgeRight ? 0x0db : 0x1ff;
}

__host__ __device__ inline unsigned edge_div(unsigned n, unsigned m, unsigned s)   // fast_div, also on the host; s = 32: divisor 1
{
    if (s >= 32) return n;
    const unsigned t = (unsigned)(((unsigned long long)m * n) >> 32);
    return (t + ((n - t) >> 1)) >> s;
}

// tile (logical index, after the XCD numbering) -> class and index of the tile within its class
__host__ __device__ inline int edge_tile_class(const ConvArgs &a, int tile, int &ct)
{
    const unsigned nb = (unsigned)a.e_nb, nt = (unsigned)a.e_nt;   // (the host keeps nt * nb < 2^32)
    const int c0 = (int)((unsigned)tile * nb / nt), c1 = (int)((unsigned)(tile + 1) * nb / nt);
    if (c1 > c0) {
        int c = 0;
        while (c < 3 && c0 >= a.e_band[c]) ++c;
        ct = c0 - (c ? a.e_band[c - 1] : 0);
        return c;
    }
    const int o = tile - c0;
    if (o < a.e_int) { ct = o; return kEdgeInterior; }
    ct = o - a.e_int;
    return kEdgeMixed;
}

// pixel `lane` of tile ct of class cls -> (b, y, x); false for the padding lanes of the last mixed tile (which get its last pixel)
__host__ __device__ inline bool edge_lane_pixel(const ConvArgs &a, int cls, int ct, int lane, int &b, int &y, int &x)
{
    int i = ct * 64 + lane;
    bool valid = true;
    if (cls == kEdgeMixed) {
        const int nm = a.e_rem[5];
        valid = i < nm;
        if (!valid) i = nm - 1;
        int c = 0;
        while (c < 4 && i >= a.e_rem[c + 1]) ++c;
        i = a.e_n[c] - (a.e_rem[c + 1] - a.e_rem[c]) + (i - a.e_rem[c]);
        cls = c;
    }
    if (cls == kEdgeTop || cls == kEdgeBottom) {
        b = (int)edge_div((unsigned)i, a.mW, a.sW);
        x = i - b * a.W;
        y = cls == kEdgeTop ? 0 : a.H - 1;
    } else if (cls == kEdgeLeft || cls == kEdgeRight) {
        b = (int)edge_div((unsigned)i, a.mH2, a.sH2);
        y = 1 + i - b * (a.H - 2);
        x = cls == kEdgeLeft ? 0 : a.W - 1;
    } else {
        b = (int)edge_div((unsigned)i, a.mI2, a.sI2);
        const int r = i - b * ((a.H - 2) * (a.W - 2));
        const int yy = (int)edge_div((unsigned)r, a.mW2, a.sW2);
        y = 1 + yy;
        x = 1 + r - yy * (a.W - 2);
    }
    return valid;
}

// LDS items of a gathered (mixed) tile: [tap row i][lane][tap column j], 9 slots per lane
constexpr int kEdgeGatherItems = 3 * 64 * 3;

// The per-frame patch a band tile stages (items of frame b start at flat b PL + org; Lf items per frame; LDS row pitch):
//   top / bottom: image rows {0, 1} / {H-2, H-1} from column -1 to column W, i.e. 2 Wp + 1 consecutive items, pitch Wp;
//   left / right: columns {0, 1} / {W-2, W-1} of image rows 0 .. H-1, 2 items per row, pitch 2.
__host__ __device__ inline void edge_band_patch(const ConvArgs &a, int cls, int &org, int &Lf, int &pitch)
{
    const bool rows = cls == kEdgeTop || cls == kEdgeBottom;
    Lf = rows ? 2 * a.Wp + 1 : 2 * a.H;
    pitch = rows ? a.Wp : 2;
    org = cls == kEdgeTop ? a.Wp - 1 : cls == kEdgeBottom ? (a.H - 1) * a.Wp - 1 : cls == kEdgeLeft ? a.Wp : a.Wp + a.W - 2;
}

// The partition of a's geometry (B, H, W, Wp, PL and the set_conv_div fields already set) into edge-class tiles: fills the e_*
// fields and returns the LDS tile the launch needs (items: the gathered layout or the longest interior run, whichever is
// larger), or 0 if the geometry is not eligible (H or W < 3, or too many tiles for the 32-bit interleave).
inline int edge_tiles_plan(ConvArgs &a)
{
    a.edge = 0;
    if (a.H < 3 || a.W < 3) return 0;
    const long B = a.B, H = a.H, W = a.W;
    const long n[5] = {B * W, B * W, B * (H - 2), B * (H - 2), B * (H - 2) * (W - 2)};
    if (n[4] + 2 * n[0] + 2 * n[2] >= (1L << 30)) return 0;
    a.e_rem[0] = 0;
    int nb = 0;
    for (int c = 0; c < 5; ++c) {
        a.e_n[c] = (int)n[c];
        a.e_rem[c + 1] = a.e_rem[c] + (int)(n[c] % 64);
        if (c < 4) { nb += (int)(n[c] / 64); a.e_band[c] = nb; }
    }
    a.e_int = (int)(n[4] / 64);
    a.e_nb = nb;
    a.e_nt = nb + a.e_int + (a.e_rem[5] + 63) / 64;
    if ((unsigned long long)a.e_nt * (unsigned long long)(a.e_nb + 1) >= (1ULL << 32)) return 0;
    auto magic = [](unsigned d, unsigned &m, unsigned &s) { if (d < 2) { m = 0; s = 32; } else fast_div_magic(d, m, s); };
    magic((unsigned)(H - 2), a.mH2, a.sH2);
    magic((unsigned)(W - 2), a.mW2, a.sW2);
    magic((unsigned)((H - 2) * (W - 2)), a.mI2, a.sI2);
    // interior tiles stage one contiguous run (first pixel - halo .. last pixel + halo), band tiles one patch per frame they
    // touch, mixed tiles the gathered layout: the longest of them
    int lt = kEdgeGatherItems;
    for (int c = kEdgeTop; c <= kEdgeRight; ++c) {
        int org, Lf, pitch;
        edge_band_patch(a, c, org, Lf, pitch);
        for (int t = 0; t < a.e_band[c] - (c ? a.e_band[c - 1] : 0); ++t) {
            int b0, b1, y, x;
            edge_lane_pixel(a, c, t, 0, b0, y, x);
            edge_lane_pixel(a, c, t, 63, b1, y, x);
            lt = lt > (b1 - b0 + 1) * Lf ? lt : (b1 - b0 + 1) * Lf;
        }
    }
    for (int t = 0; t < a.e_int; ++t) {
        int b0, y0, x0, b1, y1, x1;
        edge_lane_pixel(a, kEdgeInterior, t, 0, b0, y0, x0);
        edge_lane_pixel(a, kEdgeInterior, t, 63, b1, y1, x1);
        const int f0 = b0 * a.PL + (y0 + 1) * a.Wp + x0, f1 = b1 * a.PL + (y1 + 1) * a.Wp + x1;
        lt = lt > f1 - f0 + 1 + 2 * (a.Wp + 1) ? lt : f1 - f0 + 1 + 2 * (a.Wp + 1);
    }
    a.edge = 1;
    return lt;
}

// Steps (pixel x tap visits, per output channel and input group) of the edge-class grid: 6 taps per full band tile, 9 per
// interior or mixed tile (padding lanes included, as the kernel issues them).
inline long edge_tiles_steps(const ConvArgs &a)
{
    return 64L * (6L * a.e_nb + 9L * (a.e_nt - a.e_nb));
}

// Workgroups are dealt to the 8 XCDs round-robin in linear launch order (x fastest) and every XCD
// has its own 4 MiB L2.  Re-number them so that the XCDs form an Xt x Xm grid over (tiles, output-
// channel blocks): XCD (kt, km) owns a contiguous range of tiles and a contiguous range of blocks and
// walks it tile-major.  Neighbouring tiles (which share halo rows) and the blocks of one tile then
// meet in one L2, the input crosses the fabric Xm times and the weights Xt times; the host picks
// the split that minimises that sum (xm_log2).  Launch order in linear id: XCD = id & 7, the slot
// within the XCD = id >> 3; XCD k receives q + (k < r) workgroups, so the logical sequence (parts in
// XCD order) is cut at exactly those counts - with uneven parts a few workgroups spill to the
// neighbouring XCD, which is harmless.
__device__ inline void xcd_partition(int xm_log2, int &tile, int &yb)
{
    const int gx = gridDim.x, gy = gridDim.y, total = gx * gy;
    const int lin = blockIdx.x + blockIdx.y * gx;
    const int xcd = lin & 7, slot = lin >> 3;
    const int q = total >> 3, r = total & 7;
    int L = xcd * q + min(xcd, r) + slot;               // bijection onto [0, total)
    const int Xm = 1 << xm_log2, Xt = 8 >> xm_log2;
    const int qt = gx / Xt, rt = gx - qt * Xt, qm = gy / Xm, rm = gy - qm * Xm;
    tile = 0; yb = 0;
    for (int k = 0; k < 8; ++k) {
        const int kt = k >> xm_log2, km = k & (Xm - 1);
        const int nt = qt + (kt < rt), nm = qm + (km < rm), cnt = nt * nm;
        if (L < cnt) {
            const int dt = L / nm;
            tile = kt * qt + min(kt, rt) + dt;
            yb = km * qm + min(km, rm) + (L - dt * nm);
            break;
        }
        L -= cnt;
    }
}

// weights_reorg stream of one layer -> wpk[MB][CG][KK][32][4] with partial tiles zero-padded.
// Source block (m0,n0) starts at m0*C*KK + TM_MIN*n0*KK and is [kk][TM_MIN][TN_MIN]
// (yolov2_weight_gen.cpp:43-67; consumed in this order by core_io.cpp:154-198).
template <typename T>
__global__ void k_repack_weights(const T *__restrict__ src, T *__restrict__ dst, int C, int N, int KK)
{
    const int CG = (C + kTn - 1) / kTn, MB = (N + kTm - 1) / kTm;
    const long n = (long)MB * CG * KK * 128;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int tn = (int)(t & 3), tm = (int)((t >> 2) & 31);
    const long r = t >> 7;
    const int tap = (int)(r % KK);
    const int cg = (int)((r / KK) % CG);
    const int mb = (int)(r / ((long)KK * CG));
    const int m0 = mb * kTm, n0 = cg * kTn;
    const int tm_min = min(kTm, N - m0), tn_min = min(kTn, C - n0);
    T v = 0;
    if (tm < tm_min && tn < tn_min)
        v = src[(long)m0 * C * KK + (long)tm_min * n0 * KK + (long)tap * tm_min * tn_min + tm * tn_min + tn];
    dst[t] = v;
}

// any KxK / stride pool with the reference's pad value (core_io.cpp:96-103), reference layout
template <typename T>
__global__ void k_pool_ref(const T *__restrict__ in, T *__restrict__ out, int C, int K, int stride, int W, int H,
                           int OW, int OH, T padv)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C * OH * OW) return;
    const int x = t % OW, y = (t / OW) % OH, c = t / (OW * OH);
    const int W8 = (W + 7) & ~7, OW8 = (OW + 7) & ~7;
    T best = padv;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            const int sy = y * stride + i, sx = x * stride + j;
            const T v = (sy < H && sx < W) ? in[((long)c * H + sy) * W8 + sx] : padv;
            if (v > best) best = v;
        }
    out[((long)c * OH + y) * OW8 + x] = best;
}

}  // namespace y2
