// kernels_calib.hpp -- the two device steps of calibration (yolo2_calib.hip): the abs-max of a float range and the
// fp32 -> int16 quantiser of the weight streams.
//
// Both are one pass over HBM (4 bytes read per element; the quantiser writes 2), so they are shaped for bandwidth: 16-byte loads
// by consecutive lanes in a grid-stride loop, a grid capped at a few workgroups per CU, and - in the reduction - one atomic per
// workgroup.  Neither is on a timed path: calibration runs once per weight set.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace y2 {

constexpr int kCalibBlock = 256;
constexpr int kCalibMaxGrid = 2048;        // 256 CUs x 8 workgroups; the rest of a large range is grid-strided
constexpr unsigned kBadPerBlockCap = 1u << 20;   // a workgroup adds at most this many non-finite values: 2048 of them cannot wrap the slot

// elements in front of the first 16-byte boundary of a float pointer (0..3)
__host__ __device__ inline long calib_head_elems(const void *p, long n)
{
    const long h = (long)((0 - ((uintptr_t)p >> 2)) & 3);
    return h < n ? h : n;
}

// Non-negative floats order like their bit patterns, so max |x| is an unsigned max of bits(x) & 0x7fffffff (-0.0 -> 0, subnormals
// keep their place).  Inf and NaN (exponent all ones) are COUNTED and left out of the maximum: a NaN would otherwise win it silently.
__device__ __forceinline__ void absmax_take(unsigned bits, unsigned &m, unsigned &bad)
{
    const unsigned a = bits & 0x7fffffffu;
    if (a >= 0x7f800000u) ++bad;
    else m = a > m ? a : m;
}

// slot[0] = max(slot[0], max |x[0..n)| as bits), slot[1] += non-finite values (saturating per workgroup).  Accumulates: the caller
// zeroes the slot when a statistic starts.  Any 4-byte-aligned x: the elements in front of the first 16-byte boundary and the up to
// three behind the last full float4 are read as scalars by workgroup 0.
__global__ __launch_bounds__(kCalibBlock) void k_absmax_f32(const float *__restrict__ x, long n, unsigned *__restrict__ slot)
{
    __shared__ unsigned s_m[kCalibBlock / 64], s_bad[kCalibBlock / 64];
    const int tid = threadIdx.x;
    const long head = calib_head_elems(x, n);
    const long nv = (n - head) >> 2;
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(x + head);
    unsigned m = 0, bad = 0;
    const long stride = (long)gridDim.x * kCalibBlock;
    for (long i = (long)blockIdx.x * kCalibBlock + tid; i < nv; i += stride) {
        const uint4 u = v[i];
        absmax_take(u.x, m, bad);
        absmax_take(u.y, m, bad);
        absmax_take(u.z, m, bad);
        absmax_take(u.w, m, bad);
    }
    if (blockIdx.x == 0) {
        const unsigned *__restrict__ xs = reinterpret_cast<const unsigned *>(x);
        const long tail0 = head + (nv << 2);
        if (tid < head) absmax_take(xs[tid], m, bad);
        if (tail0 + tid < n && tid < 4) absmax_take(xs[tail0 + tid], m, bad);
    }
    // wavefront: butterfly over the 64 lanes (cross-lane moves, no LDS), then the four wavefronts through LDS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned om = __shfl_xor(m, off, 64), ob = __shfl_xor(bad, off, 64);
        m = om > m ? om : m;
        bad += ob;
    }
    if ((tid & 63) == 0) { s_m[tid >> 6] = m; s_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kCalibBlock / 64; ++w) { m = s_m[w] > m ? s_m[w] : m; bad += s_bad[w]; }
        atomicMax(&slot[0], m);
        if (bad) atomicAdd(&slot[1], bad < kBadPerBlockCap ? bad : kBadPerBlockCap);
    }
}

// int16 = round(x * 2^q), the rule of the network input (yolo2_model.cpp:257-273; orc_quantize_input restates it): the product in
// fp32, clamped, rounded half AWAY from zero (llroundf) - with the clamp symmetric, +-32767, because a bias of -32768 does not fit
// the packed accumulators of the int16 pass.  `clamped` counts the values whose rounded product lay outside +-32767
// (|x * 2^q| >= 32767.5: below that the reference's clamp-then-round gives 32767 as plain rounding does; a NaN counts and becomes 0).
__device__ __forceinline__ short quantize_one(float x, float scale, unsigned &clamped)
{
    float v = __fmul_rn(x, scale);
    if (!(fabsf(v) < 32767.5f)) {
        ++clamped;
        v = v != v ? 0.f : (v > 0.f ? 32767.f : -32767.f);
    }
    return (short)(int)roundf(v);
}

// out[i] = quantize(x[i]) for i in [0, n).  16-byte loads / 8-byte stores where x and out agree on where their vectors start (the
// layers of the two resident streams do: same element order, same offsets), scalars otherwise.
__global__ __launch_bounds__(kCalibBlock) void k_quantize_i16(const float *__restrict__ x, short *__restrict__ out, long n, int q,
                                                               unsigned *__restrict__ clamped_slot)
{
    const int tid = threadIdx.x;
    const float scale = ldexpf(1.0f, q);
    long head = calib_head_elems(x, n);
    if (((0 - ((uintptr_t)out >> 1)) & 3) != ((0 - ((uintptr_t)x >> 2)) & 3)) head = n;   // vectors would not line up: all scalar
    const long nv = (n - head) >> 2;
    const float4 *__restrict__ v = reinterpret_cast<const float4 *>(x + head);
    short4 *__restrict__ o = reinterpret_cast<short4 *>(out + head);
    unsigned clamped = 0;
    const long gtid = (long)blockIdx.x * kCalibBlock + tid, stride = (long)gridDim.x * kCalibBlock;
    for (long i = gtid; i < nv; i += stride) {
        const float4 f = v[i];
        short4 r;
        r.x = quantize_one(f.x, scale, clamped);
        r.y = quantize_one(f.y, scale, clamped);
        r.z = quantize_one(f.z, scale, clamped);
        r.w = quantize_one(f.w, scale, clamped);
        o[i] = r;
    }
    const long tail0 = head + (nv << 2);
    for (long i = gtid; i < head; i += stride) out[i] = quantize_one(x[i], scale, clamped);
    for (long i = tail0 + gtid; i < n; i += stride) out[i] = quantize_one(x[i], scale, clamped);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) clamped += __shfl_xor(clamped, off, 64);
    if ((tid & 63) == 0 && clamped) atomicAdd(clamped_slot, clamped);
}

}  // namespace y2
