// kernels_i8.hpp -- the int8 pass on the i8 matrix cores (yolo2_int8.hip launches everything here).
// (kernels_i8_front.hpp, which includes this file, holds the images entries' kernel from image bytes to layer 1.)
//
// Arithmetic (include/yolo2_hip.h "int8 pass"): acc = bias32 + sum(w8 * x8) in int32, leaky = acc / 10 truncating on the accumulator,
// one rounding shift per output channel down to the int8 output, or - layer 30 - (float)acc scaled by a power of two.  The int32 sum
// is exact, so tiling and k order change no bit: every kernel here is held to a few lines of numpy by equality.
//
// Layouts.  Activations are channel-innermost int8, [frame][y][x][Cp] with Cp = the channels rounded up to 32 (one k step of
// v_mfma_i32_32x32x32_i8; pad channels hold zeros) and no spatial border: a tap that leaves the image is staged as zeros.  Weights
// are packed once per load into the order the kernel stages them, [tap][chunk of 32 channels][output channel][32 bytes], output
// channels padded with zeros to the launch's channel tile, so the tail of no tile leaves its buffer.
//
// Fragment map of v_mfma_i32_32x32x32_i8 as this file uses it: lane l holds row (A) / column (B) l & 31 and the 16 k values
// 16 * (l >> 5) + j in byte j of its four operand registers; the result has the column on lane & 31 and row
// (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) in register reg.  A is the weights and B the pixels, so a lane ends up with one pixel
// and groups of four consecutive output channels: four bytes, one store.  The k order inside a step is irrelevant to an integer
// sum as long as A and B agree on it; rows, columns and the result map are pinned by tests/test_gpu_i8.py with identity weights and
// an asymmetric input.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace y2 {

typedef int i8frag __attribute__((ext_vector_type(4)));     // 16 int8: one A or B operand of the MFMA
typedef int i32x16 __attribute__((ext_vector_type(16)));    // its 32 x 32 int32 result, 16 values per lane

constexpr int kI8Granule = 32;   // channels per k step; the channel stride of every int8 tensor is a multiple of it

struct ConvI8Args {
    const signed char *in;   // [P][Cpi]
    const signed char *w;    // [K*K][CC][Np][32]
    const int *bias;         // [Np]
    const int *sh;           // [Np]: the rounding shift s, or - float output - Qin + Qw of the channel
    void *out;               // int8: [P][ocs], already at the layer's channel offset; float: dense [B][N][H][W]
    int CC;                  // 32-channel chunks of the input tensor (Cpi = 32 * CC)
    int K, H, W, P;          // P = frames * H * W pixels
    int N, Np, ocs, leaky;
};

// acc -> int8 by the rule of the header: leaky on the accumulator, rounding shift (or a left shift for s <= 0), saturation
__device__ __forceinline__ int i8_requant(int acc, int s, int leaky)
{
    if (leaky && acc < 0) acc /= 10;
    const long long y = s > 0 ? (((long long)acc + (1ll << (s - 1))) >> s) : ((long long)acc << (-s));
    return (int)(y < -128 ? -128 : (y > 127 ? 127 : y));
}

// Implicit-GEMM conv, 1x1 or 3x3 with stride 1 and "same" padding.  256 threads = four wavefronts as WM x (4 / WM); a wavefront owns
// MI x PI tiles of 32 output channels x 32 pixels.  Pixels are the flat index over frames, rows and columns, so any H, W and batch
// fill the tiles.  Per k step (one tap, 32 channels) the workgroup stages its weight rows and its pixels' channel bytes in LDS with
// 16-byte loads - the next step's are in flight while this one's MFMAs run - and every wavefront reads its fragments as 16 bytes per
// lane.
template <int WM, int MI, int PI, bool FOUT>
__global__ __launch_bounds__(256) void k_conv_i8(const ConvI8Args a)
{
    constexpr int WP = 4 / WM, BM = WM * MI * 32, BP = WP * PI * 32;
    constexpr int UA = (BM * 2 + 255) / 256, UB = BP * 2 / 256;   // 16-byte units per thread
    static_assert(BP * 2 % 256 == 0, "pixel tile");
    __shared__ int4 sA[BM * 2], sB[BP * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave % WM, wp = wave / WM;
    const int p0 = blockIdx.x * BP, m0 = blockIdx.y * BM;
    const int HW = a.H * a.W, pad = a.K >> 1, KK = a.K * a.K, Cpi = a.CC * 32;

    // this thread's pixels of the B tile: unit u = tid + 256 * i is half (u & 1) of pixel u >> 1
    int py[UB], px[UB];
    const signed char *psrc[UB];
#pragma unroll
    for (int i = 0; i < UB; ++i) {
        const int u = tid + 256 * i, p = p0 + (u >> 1);
        if (p < a.P) {
            const int r = p % HW;
            py[i] = r / a.W;
            px[i] = r - py[i] * a.W;
        } else {
            py[i] = -4;   // no tap of it is inside the image
            px[i] = -4;
        }
        psrc[i] = a.in + (long)p * Cpi + (u & 1) * 16;
    }

    int4 ra[UA], rb[UB];
    auto fetch = [&](int tap, int cc) {
        const int dy = tap / a.K - pad, dx = tap - (tap / a.K) * a.K - pad;
#pragma unroll
        for (int i = 0; i < UB; ++i) {
            const int sy = py[i] + dy, sx = px[i] + dx;
            const bool ok = sy >= 0 && sy < a.H && sx >= 0 && sx < a.W;
            rb[i] = ok ? *reinterpret_cast<const int4 *>(psrc[i] + ((long)dy * a.W + dx) * Cpi + cc * 32) : make_int4(0, 0, 0, 0);
        }
        const int4 *wsrc = reinterpret_cast<const int4 *>(a.w + ((long)(tap * a.CC + cc) * a.Np + m0) * 32);
#pragma unroll
        for (int i = 0; i < UA; ++i) {
            const int u = tid + 256 * i;
            if (u < BM * 2) ra[i] = wsrc[u];
        }
    };

    i32x16 acc[MI][PI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int pi = 0; pi < PI; ++pi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][pi][r] = 0;

    int tap = 0, cc = 0;
    fetch(0, 0);
    const int steps = KK * a.CC;
    for (int k = 0; k < steps; ++k) {
#pragma unroll
        for (int i = 0; i < UB; ++i) sB[tid + 256 * i] = rb[i];
#pragma unroll
        for (int i = 0; i < UA; ++i) {
            const int u = tid + 256 * i;
            if (u < BM * 2) sA[u] = ra[i];
        }
        __syncthreads();
        if (++cc == a.CC) { cc = 0; ++tap; }
        if (k + 1 < steps) fetch(tap, cc);
        i8frag fa[MI], fb[PI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int4 v = sA[((wm * MI + mi) * 32 + (lane & 31)) * 2 + (lane >> 5)];
            fa[mi] = i8frag{v.x, v.y, v.z, v.w};
        }
#pragma unroll
        for (int pi = 0; pi < PI; ++pi) {
            const int4 v = sB[((wp * PI + pi) * 32 + (lane & 31)) * 2 + (lane >> 5)];
            fb[pi] = i8frag{v.x, v.y, v.z, v.w};
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int pi = 0; pi < PI; ++pi) acc[mi][pi] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[mi], fb[pi], acc[mi][pi], 0, 0, 0);
        __syncthreads();
    }

    // epilogue: this lane's pixel of each tile, output channels in groups of four
    const int ocw = (a.N + 31) & ~31;
#pragma unroll
    for (int pi = 0; pi < PI; ++pi) {
        const int p = p0 + (wp * PI + pi) * 32 + (lane & 31);
        if (p >= a.P) continue;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = m0 + (wm * MI + mi) * 32 + 8 * g + 4 * (lane >> 5);
                const int4 b4 = *reinterpret_cast<const int4 *>(a.bias + ch), s4 = *reinterpret_cast<const int4 *>(a.sh + ch);
                const int bb[4] = {b4.x, b4.y, b4.z, b4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
                if (FOUT) {
                    const int f = p / HW, r = p - f * HW;
                    float *o = reinterpret_cast<float *>(a.out) + ((long)f * a.N + ch) * HW + r;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ch + j < a.N) {
                            int v = acc[mi][pi][4 * g + j] + bb[j];
                            if (a.leaky && v < 0) v /= 10;
                            o[(long)j * HW] = __fmul_rn((float)v, ldexpf(1.0f, -ss[j]));
                        }
                } else if (ch < ocw) {
                    unsigned w = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w |= (unsigned)(i8_requant(acc[mi][pi][4 * g + j] + bb[j], ss[j], a.leaky) & 0xff) << (8 * j);
                    *reinterpret_cast<unsigned *>(reinterpret_cast<signed char *>(a.out) + (long)p * a.ocs + ch) = w;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ the small kernels of the pass

// the input rule of the header: x8 = clamp(round_half_away(x * scale), -128, 127), NaN -> 0; scale = 2^act_q[0].  The one definition
// behind k_i8_quant_input and k_i8_front_pix (kernels_i8_front.hpp).
__device__ __forceinline__ int i8_quant_input(float x, float scale)
{
    const float v = roundf(__fmul_rn(x, scale));
    return (int)(v != v ? 0.f : fminf(fmaxf(v, -128.f), 127.f));
}

// x8 = i8_quant_input(x, 2^q) of float frames [B][3][HW] -> [B * HW][32], channels 3..31 zero
__global__ __launch_bounds__(256) void k_i8_quant_input(const float *__restrict__ frames, signed char *__restrict__ out, int q, int HW, long n)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long f = t / HW, r = t - f * HW;
    const float scale = ldexpf(1.0f, q);
    unsigned w = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) w |= (unsigned)(i8_quant_input(frames[(f * 3 + c) * HW + r], scale) & 0xff) << (8 * c);
    int4 *o = reinterpret_cast<int4 *>(out + t * 32);
    o[0] = make_int4((int)w, 0, 0, 0);
    o[1] = make_int4(0, 0, 0, 0);
}

__device__ __forceinline__ int i8_max4(int a, int b)
{
    int r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = (signed char)(a >> (8 * j)), y = (signed char)(b >> (8 * j));
        r |= ((x > y ? x : y) & 0xff) << (8 * j);
    }
    return r;
}

// 2x2 max, stride 2: [B][H][W][Cp] -> [B][H/2][W/2][Cp]; one thread per 16 channels of an output pixel
__global__ __launch_bounds__(256) void k_i8_pool(const signed char *__restrict__ in, signed char *__restrict__ out, int H, int W, int Cp, long n)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int G = Cp >> 4, OH = H >> 1, OW = W >> 1;
    const int g = (int)(t % G);
    const long op = t / G;
    const int ox = (int)(op % OW), oy = (int)((op / OW) % OH);
    const long f = op / ((long)OW * OH);
    const signed char *src = in + ((f * H + 2 * oy) * W + 2 * ox) * Cp + g * 16;
    int4 m = *reinterpret_cast<const int4 *>(src);
    const long offs[3] = {(long)Cp, (long)W * Cp, (long)(W + 1) * Cp};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int4 v = *reinterpret_cast<const int4 *>(src + offs[k]);
        m = make_int4(i8_max4(m.x, v.x), i8_max4(m.y, v.y), i8_max4(m.z, v.z), i8_max4(m.w, v.w));
    }
    *reinterpret_cast<int4 *>(out + op * Cp + g * 16) = m;
}

// the legacy Darknet reorg of the logical [64][26][26] tensor into channels [0, 256) of the concat tensor
__global__ __launch_bounds__(256) void k_i8_reorg(const signed char *__restrict__ in, signed char *__restrict__ out, int B, int ics, int ocs)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * 256 * 169) return;
    const int b = t / (256 * 169), o = t - b * (256 * 169);
    const ReorgSrc s = reorg_src(o);
    const int oc = o / 169, orr = o - oc * 169;
    out[((long)b * 169 + orr) * ocs + oc] = in[((long)b * 676 + s.sy * 26 + s.sx) * ics + s.sc];
}

// dense int8 [B][C][HW] -> [B * HW][Cp], pad channels zero (the driver tier's input)
__global__ __launch_bounds__(256) void k_i8_pack_nchw(const signed char *__restrict__ in, signed char *__restrict__ out, int C, int Cp, int HW, long n)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int c = (int)(t % Cp);
    const long p = t / Cp, f = p / HW, r = p - f * HW;
    out[t] = c < C ? in[(f * C + c) * HW + r] : (signed char)0;
}

// channels [0, C) of a [B * HW][cs] tensor (already at its channel offset) -> dense [B][C][HW]
__global__ __launch_bounds__(256) void k_i8_unpack_nchw(const signed char *__restrict__ in, signed char *__restrict__ out, int C, int cs, int HW, long n)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long r = t % HW, c = (t / HW) % C, f = t / ((long)HW * C);
    out[t] = in[(f * HW + r) * cs + c];
}

// natural [N][C][KK] int8 weights -> [KK][CC][Np][32], zeros where the output or the input channel is padding
__global__ __launch_bounds__(256) void k_i8_pack_weights(const signed char *__restrict__ w, signed char *__restrict__ out, int N, int C, int KK, int CC,
                                                         int Np, long n)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int kb = (int)(t & 31);
    const long row = t >> 5;
    const int m = (int)(row % Np), cc = (int)((row / Np) % CC), tap = (int)(row / ((long)Np * CC));
    const int c = cc * 32 + kb;
    out[t] = (m < N && c < C) ? w[((long)m * C + c) * KK + tap] : (signed char)0;
}

constexpr int kI8NoQ = -128;   // k_quantize_i8's mark for an output channel no Q in -8..24 holds (or a non-finite weight)

// The weight quantiser, one workgroup per output channel m of one conv layer.  wf is the layer's slice of the resident fp32 stream
// in the reference's tiled order (blocks of 32 output x 4 input channels, [tap][tm][tn]).  It takes the channel's max |w|, picks
// Qw = the largest q in -8..24 with max * 2^q < 127.5 (in double; 24 for an all-zero channel) and writes, in natural [N][C][KK]
// order, w8 = clamp(round_half_away(w * 2^Qw), -127, 127), and bias32 = round_half_away(b * 2^(qin + Qw)) in double.
__global__ __launch_bounds__(256) void k_quantize_i8(const float *__restrict__ wf, const float *__restrict__ bf, signed char *__restrict__ w8,
                                                     int *__restrict__ bias32, int *__restrict__ qw_out, int N, int C, int KK, int qin)
{
    __shared__ unsigned s_m[4], s_bad[4];
    __shared__ int s_q;
    const int m = blockIdx.x, tid = threadIdx.x;
    const int mb0 = m / 32 * 32, tm = min(32, N - mb0), per = C * KK;
    auto src = [&](int e) {   // natural element e = c * KK + tap of channel m -> its place in the tiled stream
        const int c = e / KK, tap = e - c * KK, n0 = c & ~3, tn = min(4, C - n0);
        return (long)mb0 * C * KK + (long)tm * n0 * KK + (long)tap * tm * tn + (long)(m - mb0) * tn + (c - n0);
    };
    unsigned mx = 0, bad = 0;
    for (int e = tid; e < per; e += 256) {
        const unsigned a = __float_as_uint(wf[src(e)]) & 0x7fffffffu;
        if (a >= 0x7f800000u) ++bad;
        else mx = a > mx ? a : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned om = __shfl_xor(mx, off, 64), ob = __shfl_xor(bad, off, 64);
        mx = om > mx ? om : mx;
        bad += ob;
    }
    if ((tid & 63) == 0) { s_m[tid >> 6] = mx; s_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { mx = s_m[w] > mx ? s_m[w] : mx; bad += s_bad[w]; }
        const double mval = (double)__uint_as_float(mx);
        int q = kI8NoQ;
        if (!bad) {
            if (mval == 0.0) q = 24;
            else
                for (int t = 24; t >= -8; --t)
                    if (mval * ldexp(1.0, t) < 127.5) { q = t; break; }
        }
        s_q = q;
        qw_out[m] = q;
        double b = 0.0;
        if (q != kI8NoQ) {
            b = (double)bf[m] * ldexp(1.0, qin + q);
            b = b != b ? 0.0 : trunc(b + (b < 0.0 ? -0.5 : 0.5));
            b = fmin(fmax(b, -2147483648.0), 2147483647.0);
        }
        bias32[m] = (int)b;
    }
    __syncthreads();
    const int q = s_q;
    const float scale = ldexpf(1.0f, q == kI8NoQ ? 0 : q);
    for (int e = tid; e < per; e += 256) {
        float v = roundf(__fmul_rn(wf[src(e)], scale));
        v = (q == kI8NoQ || v != v) ? 0.f : fminf(fmaxf(v, -127.f), 127.f);
        w8[(long)m * per + e] = (signed char)(int)v;
    }
}

}  // namespace y2
