// quant.h -- the one place where a float becomes a sample (the definition: moephoto_amd/quant.py), shared by every quantising edge: the fold's
// sample edges in stitch.hip, to_output_kernel / to_output3_kernel in misc_kernels.hip and to_output_luma_kernel in luma.hip, so that a fused edge and its unfused
// composition give the same bytes by construction.
//     DITHER = false   today's quantiser, expression for expression: v * S, clamp to [0, top], NaN = 0, truncate (S = 2^bits, top = S - 1)
//     DITHER = true    t = fl32(v * S);  u = fl32(t + T / 128);  the same clamp and truncation.  T = 64 ('round') or 2 * B8[y & 7][x & 7] + 1 ('ordered': the 8 x 8 Bayer
//                      matrix, an odd numerator 1 .. 127), picked by a block-uniform flag; S = 2^bits or 2^bits - 1 (unit scale, the inverse of the 8-bit reader's / 255).
// The product and the sum are two separately rounded fp32 operations (with S = 255 an FMA gives other bits): __fmul_rn / __fadd_rn under fp contract(off), and the empty
// asm statements keep each result in its register, as stitch_mix_mul and luma.h do.  T / 128 is exact in fp32.
// x, y are the sample's coordinates in the plane or image being written; the interleaved channels of a pixel share one threshold.  A vector-path thread's eight pixels
// start at a multiple of 8, so x & 7 is a constant per unrolled element and the eight thresholds are one matrix row chosen by y & 7: the closed form below folds to a few
// bit operations on y per row -- no table, no LDS.
#pragma once
#include "common.h"

// B8[y][x] = sum_{i < 3} (((x_i ^ y_i) << (2 (2 - i) + 1)) | (y_i << (2 (2 - i)))), x_i = bit i of x & 7: the recursion B2 = [[0, 2], [3, 1]], B2n = [[4B, 4B + 2], [4B + 3, 4B + 1]]
__device__ __forceinline__ unsigned quant_bayer8(int x, int y)
{
    const unsigned xy = (unsigned)(x ^ y) & 7u, yy = (unsigned)y & 7u;
    return ((xy & 1u) << 5) | ((yy & 1u) << 4) | ((xy & 2u) << 2) | ((yy & 2u) << 1) | ((xy & 4u) >> 1) | ((yy & 4u) >> 2);
}

// the threshold numerator T of the definition
__device__ __forceinline__ unsigned quant_threshold(bool ordered, int x, int y) { return ordered ? 2u * quant_bayer8(x, y) + 1u : 64u; }

template <typename TD, bool DITHER>
__device__ __forceinline__ TD quant_sample(float v, bool f16, float S, float top, bool ordered, int x, int y)
{
    if (f16) v = (float)(half_t)v;                       // what the fp16 canvas held
    if constexpr (DITHER) {
#pragma clang fp contract(off)
        float t = __fmul_rn(v, S);
        asm("" : "+v"(t));
        v = __fadd_rn(t, (float)quant_threshold(ordered, x, y) * (1.f / 128.f));
        asm("" : "+v"(v));
        v = fminf(fmaxf(v, 0.f), top);
    } else {
        v = v * S;                                       // to_output_kernel: image * quant, clamp_(0, quant - 1), truncate
        v = fminf(fmaxf(v, 0.f), S - 1.f);               // (top is S - 1 here, formed where the undithered kernels have always formed it)
    }
    if (!(v == v)) v = 0.f;
    return (TD)(int)v;
}

// What an edge holds of its quantiser: the one float of today's kernels, or the dithered form's three values (QuantDither, common.h)
struct QuantNone {};          // (what an edge that reads its one float elsewhere holds instead of a QuantDither)
template <bool DITHER> struct Quant;
template <> struct Quant<false> {
    float quant;
    __device__ __forceinline__ float S() const { return quant; }
    __device__ __forceinline__ float top() const { return 0.f; }          // (unused: quant_sample<.., false> forms S - 1 itself)
    __device__ __forceinline__ bool ordered() const { return false; }
};
template <> struct Quant<true> {
    QuantDither d;
    __device__ __forceinline__ float S() const { return d.S; }
    __device__ __forceinline__ float top() const { return d.top; }
    __device__ __forceinline__ bool ordered() const { return d.ordered != 0; }
};

template <typename TD, bool DITHER>
__device__ __forceinline__ TD quant_sample(float v, bool f16, const Quant<DITHER>& q, int x, int y)
{
    return quant_sample<TD, DITHER>(v, f16, q.S(), q.top(), q.ordered(), x, y);
}
