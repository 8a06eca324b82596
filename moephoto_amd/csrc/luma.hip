// luma.hip -- the two ends of a luma-only step on an RGB image (moe_luma_split, moe_luma_merge; the definition: moephoto_amd/luma.py, the arithmetic: luma.h).
// None of the SR / DN nets convolves planes jointly, so a colour image needs one pass through the net, not three: the split gives Y' (and alpha behind it) for the net
// and Cb / Cr as two fp32 planes that go to the output's size through moe_resize; the merge puts the planes back.  The reference has no counterpart: it sends every
// plane through the net (python/runSR.py:37-40).  The merge of a chain whose last fold can write the result itself is stitch.hip's LumaEdge; this file's merge serves the
// chains whose Y' is a canvas (an ensemble, a blended DN, a step that is not last).
#include "luma.h"
#include "quant.h"
#include <type_traits>
#include "../../include/moephoto_amd.h"

namespace {

// One thread = eight consecutive pixels of one row, rows strided over gridDim.y.  vec: unit column stride, base and the plane / row pitches multiples of 16 bytes -- a
// whole run is then one (fp16) or two (fp32) 16-byte loads per plane; elsewhere, and at the ragged end of a row, element by element.
template <typename T>
__global__ __launch_bounds__(256) void to_float_luma_kernel(const T* __restrict__ src, long long sC, long long sH, long long sW, int C, int H, int W, int rp, int vec,
                                                            LumaCoef k, T* __restrict__ dst_y, float* __restrict__ dst_c)
{
    const int X0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (X0 >= W) return;
    const int n = min(8, W - X0);
    const bool v16 = vec && n == 8;
    const long long HW = (long long)H * W;
    for (int Y = blockIdx.y; Y < H; Y += gridDim.y) {
        const T* row = src + Y * sH + X0 * sW;
        T r[8], g[8], b[8];
        luma_load8(row + rp * sC, sW, v16, n, r);
        luma_load8(row + sC, sW, v16, n, g);
        luma_load8(row + (2 - rp) * sC, sW, v16, n, b);
        StitchRun<T, 8> oy;
        StitchRun<float, 8> ob, orr;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float y;
            luma_split_px(k, (float)r[e], (float)g[e], (float)b[e], y, ob.e[e], orr.e[e]);
            oy.e[e] = (T)y;
        }
        const long long at = (long long)Y * W + X0;
        stitch_store_n(dst_y + at, oy, n);
        stitch_store_n(dst_c + at, ob, n);
        stitch_store_n(dst_c + HW + at, orr, n);
        if (C == 4) {          // alpha rides as Y's second plane
            luma_load8(row + 3 * sC, sW, v16, n, r);
            StitchRun<T, 8> oa;
#pragma unroll
            for (int e = 0; e < 8; ++e) oa.e[e] = r[e];
            stitch_store_n(dst_y + HW + at, oa, n);
        }
    }
}

// The merge on dense planes: y = CT - 2 planes of H x W (T), c = Cb, Cr (fp32).  Dense, so the planes are flat arrays of HW elements: one thread = eight consecutive
// elements.  TD == T: dst = the canvas (CT, H, W); else dst = (H, W, CT) interleaved samples through to_output_kernel's quantiser, each value rounded to T first.
// DITHER (to_output_luma_dither_kernel, the sample form only): quant.h's rounding / ordered-dither quantiser at the pixel's coordinates (i % W, i / W) -- the bytes of the fold's
// dithered LumaEdge.
template <typename T, typename TD, int CT, bool DITHER>
__device__ __forceinline__ void to_output_luma_body(const T* __restrict__ y, const float* __restrict__ c, long long HW, int rp, const LumaCoef& k, const Quant<DITHER>& q, int W, TD* __restrict__ dst)
{
    constexpr bool SAMPLE = !std::is_same<T, TD>::value;
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= HW) return;
    const int n = (int)min(8ll, HW - i0);
    auto aligned = [&](const void* p) { return n == 8 && ((uintptr_t)p & 15) == 0; };
    T yv[8], av[8];
    float cb[8], cr[8];
    luma_load8(y + i0, 1, aligned(y + i0), n, yv);
    luma_load8(c + i0, 1, aligned(c + i0), n, cb);
    luma_load8(c + HW + i0, 1, aligned(c + HW + i0), n, cr);
    if constexpr (CT == 4) luma_load8(y + HW + i0, 1, aligned(y + HW + i0), n, av);
    T o[CT][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) luma_merge_planes<T>(k, (float)yv[e], cb[e], cr[e], rp, o[0][e], o[1][e], o[2][e]);
    if constexpr (CT == 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[3][e] = luma_canon(av[e]);
    }
    if constexpr (SAMPLE) {
        StitchRun<TD, 8 * CT> s;
        int px[8], py[8];          // (DITHER only: the eight pixels' coordinates, one division per thread)
        if constexpr (DITHER) {
            px[0] = (int)(i0 % W); py[0] = (int)(i0 / W);
#pragma unroll
            for (int e = 1; e < 8; ++e) {
                const bool wrap = px[e - 1] + 1 == W;
                px[e] = wrap ? 0 : px[e - 1] + 1; py[e] = py[e - 1] + (wrap ? 1 : 0);
            }
        }
#pragma unroll
        for (int p = 0; p < CT; ++p)
#pragma unroll
            for (int e = 0; e < 8; ++e) s.e[e * CT + p] = quant_sample<TD>((float)o[p][e], false, q, DITHER ? px[e] : 0, DITHER ? py[e] : 0);
        stitch_store_n(dst + i0 * CT, s, n);
    } else {
#pragma unroll
        for (int p = 0; p < CT; ++p) {
            StitchRun<T, 8> s;
#pragma unroll
            for (int e = 0; e < 8; ++e) s.e[e] = o[p][e];
            stitch_store_n(dst + p * HW + i0, s, n);
        }
    }
}

template <typename T, typename TD, int CT>
__global__ __launch_bounds__(256) void to_output_luma_kernel(const T* __restrict__ y, const float* __restrict__ c, long long HW, int rp, LumaCoef k, float quant, TD* __restrict__ dst)
{
    to_output_luma_body<T, TD, CT, false>(y, c, HW, rp, k, Quant<false>{quant}, 0, dst);
}

template <typename T, typename TD, int CT>
__global__ __launch_bounds__(256) void to_output_luma_dither_kernel(const T* __restrict__ y, const float* __restrict__ c, long long HW, int rp, LumaCoef k, QuantDither d, int W, TD* __restrict__ dst)
{
    to_output_luma_body<T, TD, CT, true>(y, c, HW, rp, k, Quant<true>{d}, W, dst);
}

template <typename T, typename TD>
void launch_luma_merge_t(const void* y, const float* c, int C, long long HW, const LumaCoef& k, int rp, float quant, void* dst, hipStream_t s, const QuantDither* dq = nullptr, int W = 0)
{
    const dim3 g((unsigned)(((HW + 7) / 8 + 255) / 256));
    if constexpr (!std::is_same<T, TD>::value) {
        if (dq) {
            if (C == 3) hipLaunchKernelGGL((to_output_luma_dither_kernel<T, TD, 3>), g, dim3(256), 0, s, (const T*)y, c, HW, rp, k, *dq, W, (TD*)dst);
            else hipLaunchKernelGGL((to_output_luma_dither_kernel<T, TD, 4>), g, dim3(256), 0, s, (const T*)y, c, HW, rp, k, *dq, W, (TD*)dst);
            return;
        }
    }
    if (C == 3) hipLaunchKernelGGL((to_output_luma_kernel<T, TD, 3>), g, dim3(256), 0, s, (const T*)y, c, HW, rp, k, quant, (TD*)dst);
    else hipLaunchKernelGGL((to_output_luma_kernel<T, TD, 4>), g, dim3(256), 0, s, (const T*)y, c, HW, rp, k, quant, (TD*)dst);
}

}  // namespace

void launch_luma_split(const void* img, int dtype, int C, long long sC, long long sH, long long sW, int H, int W, const LumaCoef& k, int rp, void* dst_y, float* dst_c, hipStream_t s)
{
    const long long V = dtype == MOE_F16 ? 8 : 4;          // elements of a 16-byte vector: base, plane and row pitch must be multiples of it
    const int vec = sW == 1 && (uintptr_t)img % 16 == 0 && sC % V == 0 && sH % V == 0;
    const dim3 g(((W + 7) / 8 + 255) / 256, H < 65535 ? H : 65535);
    if (dtype == MOE_F16) hipLaunchKernelGGL((to_float_luma_kernel<half_t>), g, dim3(256), 0, s, (const half_t*)img, sC, sH, sW, C, H, W, rp, vec, k, (half_t*)dst_y, dst_c);
    else hipLaunchKernelGGL((to_float_luma_kernel<float>), g, dim3(256), 0, s, (const float*)img, sC, sH, sW, C, H, W, rp, vec, k, (float*)dst_y, dst_c);
}

// quant == 0: dst = the canvas (C, H, W) of `dtype`; else dst = (H, W, C) of dst_dtype MOE_U8 / MOE_U16
void launch_luma_merge(const void* y, int dtype, const float* c, int C, int H, int W, const LumaCoef& k, int rp, float quant, void* dst, int dst_dtype, hipStream_t s, const QuantDither* dq)
{
    const long long HW = (long long)H * W;
    const bool f16 = dtype == MOE_F16;
    if (quant == 0.f) {
        if (f16) launch_luma_merge_t<half_t, half_t>(y, c, C, HW, k, rp, quant, dst, s);
        else launch_luma_merge_t<float, float>(y, c, C, HW, k, rp, quant, dst, s);
    } else if (dst_dtype == MOE_U8) {
        if (f16) launch_luma_merge_t<half_t, uint8_t>(y, c, C, HW, k, rp, quant, dst, s, dq, W);
        else launch_luma_merge_t<float, uint8_t>(y, c, C, HW, k, rp, quant, dst, s, dq, W);
    } else {
        if (f16) launch_luma_merge_t<half_t, uint16_t>(y, c, C, HW, k, rp, quant, dst, s, dq, W);
        else launch_luma_merge_t<float, uint16_t>(y, c, C, HW, k, rp, quant, dst, s, dq, W);
    }
}
