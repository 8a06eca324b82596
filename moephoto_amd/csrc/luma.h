// luma.h -- the per-pixel arithmetic of the luma-only steps (the definition: moephoto_amd/luma.py), shared by the split / merge kernels of luma.hip and the fold's
// LumaEdge in stitch.hip, so that the fused merge and the unfused one give the same bits by construction.
// All arithmetic is fp32; every product and every sum is rounded separately, in the order the definition writes them: the empty asm statements keep each result in its
// register, so that no product is fused into the sum behind it (an FMA rounds once) nor into a conversion to fp16 (v_fma_mixlo_f16), as stitch_mix_mul does.
#pragma once
#include "common.h"
#include "run_store.h"

__device__ __forceinline__ float luma_mul(float a, float b)
{
#pragma clang fp contract(off)
    float p = __fmul_rn(a, b);
    asm("" : "+v"(p));
    return p;
}

__device__ __forceinline__ float luma_add(float a, float b)
{
#pragma clang fp contract(off)
    float p = __fadd_rn(a, b);
    asm("" : "+v"(p));
    return p;
}

// y = (kr r + kg g) + kb b;  cb = (b - y) ib;  cr = (r - y) ir  (cb / cr from the unrounded y)
__device__ __forceinline__ void luma_split_px(const LumaCoef& k, float r, float g, float b, float& y, float& cb, float& cr)
{
    y = luma_add(luma_add(luma_mul(k.kr, r), luma_mul(k.kg, g)), luma_mul(k.kb, b));
    cb = luma_mul(luma_add(b, -y), k.ib);
    cr = luma_mul(luma_add(r, -y), k.ir);
}

// colour 0: r' = y + er cr;  2: b' = y + eb cb;  1: g' = y - (gr cr + gb cb)
__device__ __forceinline__ float luma_merge_px(const LumaCoef& k, float y, float cb, float cr, int colour)
{
    if (colour == 0) return luma_add(y, luma_mul(k.er, cr));
    if (colour == 2) return luma_add(y, luma_mul(k.eb, cb));
    return luma_add(y, -luma_add(luma_mul(k.gr, cr), luma_mul(k.gb, cb)));
}

// the colour of output plane p (0 .. 2) when red is plane rp (0: 'rgb', 2: 'bgr')
__device__ __forceinline__ int luma_colour(int p, int rp) { return p == 1 ? 1 : (p == rp ? 0 : 2); }

// A NaN leaves the merge as THE quiet NaN of T (0x7e00 / 0x7fc00000).  Whose sign and payload an operation on two NaNs hands on, and what a negation folded into a
// subtraction does to them, is the hardware's and the compiler's choice, kernel by kernel -- and the fused and the unfused merge owe each other the same bytes.
template <typename T>
__device__ __forceinline__ T luma_canon(T v) { return v == v ? v : (T)__builtin_nanf(""); }

// the three colour planes of one pixel, rounded to T, in the order rp says
template <typename T>
__device__ __forceinline__ void luma_merge_planes(const LumaCoef& k, float y, float cb, float cr, int rp, T& p0, T& p1, T& p2)
{
    const T r = luma_canon((T)luma_merge_px(k, y, cb, cr, 0)), b = luma_canon((T)luma_merge_px(k, y, cb, cr, 2));
    p0 = rp == 0 ? r : b;
    p1 = luma_canon((T)luma_merge_px(k, y, cb, cr, 1));
    p2 = rp == 0 ? b : r;
}

// (the quantiser of the sample forms is quant.h's quant_sample)

// Eight elements from p with element stride sW; vec: p is 16-byte aligned and sW == 1 (whole runs only).  n < 8: the ragged end of a row, the last element repeated.
template <typename T>
__device__ __forceinline__ void luma_load8(const T* p, long long sW, bool vec, int n, T (&v)[8])
{
    if (vec) {
        typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int N = 16 / sizeof(T);
#pragma unroll
        for (int k = 0; k < 8 / N; ++k) {
            const vec_t q = *(const vec_t*)(p + k * N);
#pragma unroll
            for (int e = 0; e < N; ++e) v[k * N + e] = q[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[min(e, n - 1) * sW];
    }
}
