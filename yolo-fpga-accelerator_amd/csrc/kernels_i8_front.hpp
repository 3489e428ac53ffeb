// kernels_i8_front.hpp -- the front of the int8 pass from image bytes (yolo2_int8.hip launches it).
//
// k_i8_front_pix<PIX> replaces four launches of the frames route - the chunk letterbox, k_i8_quant_input, layer 0 (k_conv_i8 with nine
// k steps that are 3/32 full) and layer 1 (k_i8_pool) - and the two 416 x 416 x 32-byte tensors between them.  It reads a chunk's
// staging buffer (LetterboxItem table + images, letterbox.hpp) and writes layer 1's tensor [frame][208][208][32].
//
// A workgroup (256 threads) owns a 32 x 32 tile of conv pixels of one frame.  It builds the quantised patch of the tile plus a
// one-pixel halo in LDS, one dword {c0, c1, c2, 0} per canvas element: lb_value_at's float through i8_quant_input, 0 outside the
// canvas (the conv's zero padding; a letterbox band inside the canvas is the quantised 0.5, and lb_value_at loads no byte there).
// Each wavefront then runs eight v_mfma_i32_32x32x32_i8, one per 32 conv pixels x 32 output channels: all 27 inputs of a pixel
// are ONE k step (front_k_tap / front_k_ch below).  Weights are the A operand, pixels the B operand, so a result column is a pixel.
//
// Pixel order: column p of a block is member p & 3 (dy = (p >> 1) & 1, dx = p & 1) of pool window p >> 2, eight windows side by
// side.  The four members of a window sit in four adjacent lanes and meet in two quad-permute DPP moves.
// Channel order: MFMA row R carries output channel front_row_channel(R), chosen so that a lane's 16 result registers are 16
// CONSECUTIVE channels (16 * (lane >> 5) + reg): a pooled pixel leaves as two 16-byte stores.
// Epilogue: max over the window on the raw accumulators FIRST, then bias, leaky, shift and saturation once per pooled value.
// bias is per channel and i8_requant is non-decreasing in acc for a fixed channel (acc / 10 truncating, the rounding shift and the
// clamp are all monotone), so requant(max(acc) + bias) == max(requant(acc + bias)): the bits of pool(conv) as the frames route makes
// them, with a quarter of the requantisations.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_i8.hpp"
#include "letterbox.hpp"

namespace y2 {

// The k map of the front's single k step, used by the kernel (pixel side) and by front_pack_weights (weight side).  Lane half h
// holds k = 16 h + j: half 0 is taps 0..4 (k = 3 tap + c, k 15 unused), half 1 is taps 5..8 (k = 16 + 3 (tap - 5) + c, k 28..31
// unused).  tap = 3 ky + kx as in the natural weight order [N][C][3][3].  An unused k has zero weights.
constexpr int kFrontTapsHalf0 = 5;
constexpr int front_k_tap(int k) { return k < 15 ? k / 3 : (k >= 16 && k < 28 ? kFrontTapsHalf0 + (k - 16) / 3 : -1); }
constexpr int front_k_ch(int k) { return k < 15 ? k % 3 : (k >= 16 && k < 28 ? (k - 16) % 3 : -1); }
// output channel of MFMA row R: result register reg of lane half h is row (reg & 3) + 8 (reg >> 2) + 4 h, i.e. channel 16 h + reg
constexpr int front_row_channel(int R) { return (R & 3) | (((R >> 3) & 3) << 2) | (((R >> 2) & 1) << 4); }

constexpr int kFrontTile = 32;                    // conv pixels per tile side
constexpr int kFrontPatch = kFrontTile + 2;       // with the halo
constexpr int kFrontPitch = 48;                   // dwords per patch row: 16 mod 32, so a block's two conv rows fall on disjoint banks
constexpr int kFrontTilesPerFrame = (416 / kFrontTile) * (416 / kFrontTile);
static_assert(416 % kFrontTile == 0 && kFrontPitch >= kFrontPatch && kFrontPitch % 32 == 16, "front tile");

// natural layer-0 weights w8 [32][3][9] -> the A fragments [channel][32 k bytes] (host side, 1 KB)
inline void front_pack_weights(const int8_t *w8, int8_t *out)
{
    for (int m = 0; m < 32; ++m)
        for (int k = 0; k < 32; ++k) out[m * 32 + k] = front_k_tap(k) < 0 ? (int8_t)0 : w8[(m * 3 + front_k_ch(k)) * 9 + front_k_tap(k)];
}

struct FrontI8Args {
    const uint8_t *lb;        // the chunk's staging buffer
    const signed char *w;     // front_pack_weights' 1 KB
    const int *bias, *sh;     // layer 0's [32]
    signed char *out;         // [frames][208][208][32]
    int q0, leaky;            // act_q[0]
};

// the kernel's body, so that a format's kernel can carry its own name (k_i8_front_pix below; kernels_i8_front_pix.hpp)
template <class PIX>
__device__ __forceinline__ void i8_front_tiles(const FrontI8Args &a)
{
    __shared__ float lbt[256];
    __shared__ unsigned patch[kFrontPatch * kFrontPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int frame = blockIdx.x / kFrontTilesPerFrame, tr = blockIdx.x % kFrontTilesPerFrame;
    const int ty0 = (tr / (416 / kFrontTile)) * kFrontTile, tx0 = (tr % (416 / kFrontTile)) * kFrontTile;

    lbt[tid] = __fdiv_rn((float)tid, 255.f);

    // this lane's part of the weight fragment, once: row lane & 31 is channel front_row_channel(lane & 31), k half h
    const int4 wv = *reinterpret_cast<const int4 *>(a.w + front_row_channel(lane & 31) * 32 + 16 * h);
    const i8frag fa = i8frag{wv.x, wv.y, wv.z, wv.w};
    __syncthreads();

    // the patch: canvas rows ty0 - 1 .. ty0 + 32, columns tx0 - 1 .. tx0 + 32
    {
        const LetterboxItem *item = reinterpret_cast<const LetterboxItem *>(a.lb) + frame;
        const LetterboxArgs la = item->a;
        const uint8_t *img = a.lb + item->off;
        const LbTable q{lbt};
        const float scale = ldexpf(1.0f, a.q0);
        for (int i = tid; i < kFrontPatch * kFrontPatch; i += 256) {
            const int py = i / kFrontPatch, px = i - py * kFrontPatch, y = ty0 - 1 + py, x = tx0 - 1 + px;
            unsigned w = 0;
            if (y >= 0 && y < 416 && x >= 0 && x < 416) {
#pragma unroll
                for (int c = 0; c < 3; ++c) w |= (unsigned)(i8_quant_input(lb_value_at<LbTable, PIX>(img, la, c, y, x, q), scale) & 0xff) << (8 * c);
            }
            patch[py * kFrontPitch + px] = w;
        }
    }

    // bias and shift of this lane's 16 channels
    int bb[16], ss[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int4 b4 = *reinterpret_cast<const int4 *>(a.bias + 16 * h + 4 * g), s4 = *reinterpret_cast<const int4 *>(a.sh + 16 * h + 4 * g);
        bb[4 * g] = b4.x; bb[4 * g + 1] = b4.y; bb[4 * g + 2] = b4.z; bb[4 * g + 3] = b4.w;
        ss[4 * g] = s4.x; ss[4 * g + 1] = s4.y; ss[4 * g + 2] = s4.z; ss[4 * g + 3] = s4.w;
    }

    // the five patch dwords of this lane's k half, relative to the top-left element of its 3 x 3 window: element i holds k = 16 h + 3 i ..
    int off[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int t0 = front_k_tap(3 * i), t1 = front_k_tap(16 + 3 * (i < 4 ? i : 3));   // (half 1 has four: its fifth is masked below)
        off[i] = h ? (t1 / 3) * kFrontPitch + t1 % 3 : (t0 / 3) * kFrontPitch + t0 % 3;
    }
    static_assert(front_k_tap(0) == 0 && front_k_tap(14) == 4 && front_k_tap(15) < 0 && front_k_tap(16) == 5 && front_k_tap(27) == 8 && front_k_tap(28) < 0,
                  "the shifts below pack five and four {c0, c1, c2, 0} dwords");
    __syncthreads();

    const int win = (lane & 31) >> 2, dy = (lane >> 1) & 1, dx = lane & 1;
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
        const int blk = wave * 8 + j, wy = blk >> 1, wx = (blk & 1) * 8 + win;   // the window inside the tile's 16 x 16
        const unsigned *p = patch + (2 * wy + dy) * kFrontPitch + 2 * wx + dx;  // top-left of the 3 x 3 (patch origin = tile origin - 1)
        const unsigned d0 = p[off[0]], d1 = p[off[1]], d2 = p[off[2]], d3 = p[off[3]], d4 = p[off[4]];
        // 3-byte elements packed densely (byte 3 of every patch dword is 0)
        const i8frag fb = i8frag{(int)(d0 | (d1 << 24)), (int)((d1 >> 8) | (d2 << 16)), (int)((d2 >> 16) | (d3 << 8)), h ? 0 : (int)d4};
        i32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
        // max over the window's four lanes (quad_perm [1,0,3,2], then [2,3,0,1]), then one requantisation per pooled value
        unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int v = acc[r];
            v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));
            v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));
            o[r >> 2] |= (unsigned)(i8_requant(v + bb[r], ss[r], a.leaky) & 0xff) << (8 * (r & 3));
        }
        if ((lane & 3) == 0) {
            const int oy = (ty0 >> 1) + wy, ox = (tx0 >> 1) + wx;
            *reinterpret_cast<int4 *>(a.out + (((long)frame * 208 + oy) * 208 + ox) * 32 + 16 * h) = make_int4((int)o[0], (int)o[1], (int)o[2], (int)o[3]);
        }
    }
}

template <class PIX>
__global__ __launch_bounds__(256) void k_i8_front_pix(const FrontI8Args a)
{
    i8_front_tiles<PIX>(a);
}

}  // namespace y2
