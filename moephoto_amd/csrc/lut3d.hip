// lut3d.hip -- the 3D LUT colour step (moe_lut3d_run; the definition: moephoto_amd/lut3d.py, transform / apply): per pixel a trilinear lookup in a 3D table whose
// lattice has non-uniform intervals -- the reference's AiLUT transform (site-packages/ailut/csrc/ailut_transform_cuda.cu; its CPU twin ailut_transform_cpu.cpp:20-113
// is the expression the definition copies) -- behind the chain's sample reader and in front of quant.h's quantiser: an edge that reads interleaved samples and writes
// interleaved samples, one launch per frame.
//
// The table on the device is one 16-byte entry {R, G, B, 0} per lattice point, red fastest (moe_lut3d_create re-lays it): a corner is one 16-byte load, the two
// red-adjacent corners are 32 contiguous bytes.  d = 33 is 575 KB: beyond LDS, it lives in L2; d = 65 is 4.4 MB and does not fit one XCD's L2.  The 3 d vertices go
// into LDS once per workgroup; a search is at most 7 steps there.
//
// One thread = eight consecutive pixels of one row, starting at a multiple of 8 (so x & 7 is the unrolled element's index and the ordered threshold folds to bit
// operations on y): its 24 samples come by vector loads where the address allows them, element by element elsewhere (a row's ragged end, a base or a width that
// leaves the run unaligned), and leave through stitch_store_n.
//
// Every product, sum and quotient is one separately rounded fp32 operation in the definition's order (luma.h's luma_mul / luma_add; the division is the correctly
// rounded one): the device's bytes are the definition's.
#include "luma.h"
#include "quant.h"

namespace {

__device__ __forceinline__ float lut_div(float a, float b)
{
#pragma clang fp contract(off)
    float q = __fdiv_rn(a, b);
    asm("" : "+v"(q));
    return q;
}

// clamp(lower_bound(v, x) - 1, 0, d - 2): the first i with v[i] >= x; a NaN finds index 0
__device__ __forceinline__ int lut_cell(const float* v, int d, float x)
{
    int lo = 0, hi = d;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return min(max(lo - 1, 0), d - 2);
}

// the fraction of x in its cell: (x - v[i]) / ((v[i + 1] - v[i]) + 1e-10f)
__device__ __forceinline__ float lut_frac(const float* v, int i, float x)
{
    const float v0 = v[i], v1 = v[i + 1];
    return lut_div(luma_add(x, -v0), luma_add(luma_add(v1, -v0), 1e-10f));
}

template <typename Src> __device__ __forceinline__ float lut_read(Src c);
template <> __device__ __forceinline__ float lut_read<uint16_t>(uint16_t c) { return (float)c * (1.f / 65536.f); }      // (exact)
template <> __device__ __forceinline__ float lut_read<uint8_t>(uint8_t c) { return lut_div((float)c, 255.f); }

template <typename Src, typename Dst, bool DITHER>
__global__ __launch_bounds__(256) void to_output_lut3d_kernel(const Src* __restrict__ src, Dst* __restrict__ dst, int H, int W, Lut3dArgs k, Quant<DITHER> q)
{
    __shared__ float vert[3 * LUT3D_MAX];
    const int d = k.d;
    for (int i = threadIdx.x; i < 3 * d; i += 256) vert[i] = k.vert[i];
    __syncthreads();
    const int runs = (W + 7) >> 3;                                   // runs of eight pixels per row
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)H * runs) return;
    const int Y = (int)(t / runs), X = (int)(t % runs) * 8;
    const int n = min(8, W - X);
    const long long at = ((long long)Y * W + X) * 3;
    StitchRun<Src, 24> in;
    if (n == 8 && ((uintptr_t)(src + at) & (alignof(StitchRun<Src, 24>) - 1)) == 0) in = *(const StitchRun<Src, 24>*)(src + at);
    else {
#pragma unroll
        for (int e = 0; e < 24; ++e) in.e[e] = e < 3 * n ? src[at + e] : (Src)0;
    }
    const float* const vr = vert, * const vg = vert + d, * const vb = vert + 2 * d;
    const bool rgb = k.rgb != 0, blend = k.blend != 0;
    const int dd = d * d;
    StitchRun<Dst, 24> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float s0 = lut_read<Src>(in.e[3 * e]), xg = lut_read<Src>(in.e[3 * e + 1]), s2 = lut_read<Src>(in.e[3 * e + 2]);
        const float xr = rgb ? s0 : s2, xb = rgb ? s2 : s0;
        const int ir = lut_cell(vr, d, xr), ig = lut_cell(vg, d, xg), ib = lut_cell(vb, d, xb);
        const float tr = lut_frac(vr, ir, xr), tg = lut_frac(vg, ig, xg), tb = lut_frac(vb, ib, xb);
        const float ur = luma_add(1.f, -tr), ug = luma_add(1.f, -tg), ub = luma_add(1.f, -tb);
        const float4* const c = k.table + (ir + d * ig + dd * ib);
        const float4 L000 = c[0], L100 = c[1], L010 = c[d], L110 = c[d + 1], L001 = c[dd], L101 = c[dd + 1], L011 = c[dd + d], L111 = c[dd + d + 1];
        const float a00 = luma_mul(ur, ug), a10 = luma_mul(tr, ug), a01 = luma_mul(ur, tg), a11 = luma_mul(tr, tg);
        const float w000 = luma_mul(a00, ub), w100 = luma_mul(a10, ub), w010 = luma_mul(a01, ub), w110 = luma_mul(a11, ub);
        const float w001 = luma_mul(a00, tb), w101 = luma_mul(a10, tb), w011 = luma_mul(a01, tb), w111 = luma_mul(a11, tb);
#define LUT_SUM(m)                                                                                                                          \
    luma_add(luma_add(luma_add(luma_add(luma_add(luma_add(luma_add(luma_mul(w000, L000.m), luma_mul(w100, L100.m)), luma_mul(w010, L010.m)), \
                                                 luma_mul(w110, L110.m)), luma_mul(w001, L001.m)), luma_mul(w101, L101.m)), luma_mul(w011, L011.m)), luma_mul(w111, L111.m))
        float yr = LUT_SUM(x), yg = LUT_SUM(y), yb = LUT_SUM(z);
#undef LUT_SUM
        if (blend) {          // RGBFilter's blend: fl32(fl32(s y) + fl32(fl32(1 - s) x))
            yr = luma_add(luma_mul(k.strength, yr), luma_mul(k.rest, xr));
            yg = luma_add(luma_mul(k.strength, yg), luma_mul(k.rest, xg));
            yb = luma_add(luma_mul(k.strength, yb), luma_mul(k.rest, xb));
        }
        const Dst R = quant_sample<Dst, DITHER>(yr, false, q, e, Y), G = quant_sample<Dst, DITHER>(yg, false, q, e, Y), B = quant_sample<Dst, DITHER>(yb, false, q, e, Y);
        o.e[3 * e] = rgb ? R : B;
        o.e[3 * e + 1] = G;
        o.e[3 * e + 2] = rgb ? B : R;
    }
    stitch_store_n(dst + at, o, n);
}

template <typename Src, typename Dst>
void launch_lut3d_t(const Src* src, int H, int W, Dst* dst, const Lut3dArgs& k, float quant, const QuantDither* dq, hipStream_t s)
{
    const long long threads = (long long)H * ((W + 7) >> 3);
    const dim3 g((unsigned)((threads + 255) / 256));
    if (dq) hipLaunchKernelGGL((to_output_lut3d_kernel<Src, Dst, true>), g, dim3(256), 0, s, src, dst, H, W, k, Quant<true>{*dq});
    else hipLaunchKernelGGL((to_output_lut3d_kernel<Src, Dst, false>), g, dim3(256), 0, s, src, dst, H, W, k, Quant<false>{quant});
}

}  // namespace

// Checked by moe_lut3d_run: H, W of 1 at least with 3 H W within an int, src_bits / bits in {8, 16}; k.table / k.vert are the handle's device copies.
void launch_lut3d(const void* src, int src_bits, int H, int W, void* dst, int bits, const Lut3dArgs& k, float quant, const QuantDither* dq, hipStream_t s)
{
    if (src_bits == 8 && bits == 8) launch_lut3d_t((const uint8_t*)src, H, W, (uint8_t*)dst, k, quant, dq, s);
    else if (src_bits == 8) launch_lut3d_t((const uint8_t*)src, H, W, (uint16_t*)dst, k, quant, dq, s);
    else if (bits == 8) launch_lut3d_t((const uint16_t*)src, H, W, (uint8_t*)dst, k, quant, dq, s);
    else launch_lut3d_t((const uint16_t*)src, H, W, (uint16_t*)dst, k, quant, dq, s);
}
