// planes_rgb.hip -- RGB frames from a chain on 4:2:0 planes (moe_planes_to_rgb; the definition: moephoto_amd/pixfmt.py, rgbCoefficients / toRGB): the Cb and Cr codes
// of a planar frame brought to luma size by chroma.hip's integer polyphase filter at scale 2, then the standard's inverse matrix in fixed point, one rounding shift per
// sample, interleaved.  No floating point anywhere: the device's bytes are the definition's.  The upsampled chroma planes never exist in memory.
//
// One workgroup of 256 threads = a tile of RGB_TW x RGB_TH luma pixels.  The clamped source windows of BOTH chroma planes -- the tile's RGB_TW / 2 x RGB_TH / 2 samples
// and RGB_LO before / RGB_HI behind them, what offsets in [-2, 1] and four taps can reach -- are read into LDS once through poly_window: the edge sample repeats there
// and neither pass holds an edge case.  Row pass (int32, poly_dot24): one thread per tile column and plane, every window row.  Column pass (int64): one thread = eight
// consecutive pixels of two consecutive rows (the two phases of one chroma row); it reads its Y' run with one 16-byte (u8: 8-byte) load where the address allows it,
// applies the matrix and stores 24 samples through stitch_store.  The tables of both axes come by value in the kernel's arguments (pixfmt.chromaTable, phases 0 and 1).
// A tile starts at even coordinates, so output column X reads chroma column X >> 1 with phase X & 1.
//
// LDS per workgroup: 2 x 22 x 128 ints + 2 x 22 x 70 samples = 28 688 bytes (u16 sources), five workgroups to a CU.  The kernel is bound by its stores: per pixel it
// reads 1.5 samples and writes 3.
#include "polyphase.h"
#include "quant.h"

namespace {

constexpr int RGB_TW = 128, RGB_TH = 32;            // the luma tile of a workgroup (tests/test_gpu_planes_rgb.py derives its edge shapes from these)
constexpr int RGB_LO = 2, RGB_HI = 4;               // window margins: off >= -2;  off + TAPS - 1 <= 1 + 3
constexpr int RGB_SW = RGB_TW / 2 + RGB_LO + RGB_HI, RGB_SH = RGB_TH / 2 + RGB_LO + RGB_HI;

template <int TAPS>
__device__ __forceinline__ void rgb_coefs(const ChromaTab& t, int p, int (&c)[TAPS])
{
#pragma unroll
    for (int j = 0; j < TAPS; ++j) c[j] = t.coef[p][j];
}

// The column pass of eight consecutive samples (polyphase.h's poly_run8 without its store): clamp((2^27 + sum_i c[i] * m[i * RGB_TW + e]) >> 28, 0, cmax)
template <int TAPS>
__device__ __forceinline__ void rgb_column8(const int (&c)[TAPS], const int* m, int cmax, int (&s)[8])
{
    long long v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 1ll << 27;
#pragma unroll
    for (int i = 0; i < TAPS; ++i) {
        const int4 a = *(const int4*)(m + i * RGB_TW), b = *(const int4*)(m + i * RGB_TW + 4);
        v[0] += (long long)c[i] * a.x; v[1] += (long long)c[i] * a.y; v[2] += (long long)c[i] * a.z; v[3] += (long long)c[i] * a.w;
        v[4] += (long long)c[i] * b.x; v[5] += (long long)c[i] * b.y; v[6] += (long long)c[i] * b.z; v[7] += (long long)c[i] * b.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = min(max((int)(v[e] >> 28), 0), cmax);
}

// The first n of eight consecutive Y' codes: one vector load where all eight exist and the address is aligned to the run, element by element elsewhere
template <typename Src>
__device__ __forceinline__ void rgb_luma8(const Src* __restrict__ p, int n, int (&y)[8])
{
    StitchRun<Src, 8> r;
    if (n == 8 && ((uintptr_t)p & (alignof(StitchRun<Src, 8>) - 1)) == 0) r = *(const StitchRun<Src, 8>*)p;
    else {
#pragma unroll
        for (int e = 0; e < 8; ++e) r.e[e] = e < n ? p[e] : (Src)0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (int)r.e[e];
}

template <typename Dst>
__device__ __forceinline__ Dst rgb_sample(long long acc, int top) { return (Dst)min(max((int)(acc >> RGB_FRAC), 0), top); }

template <typename Src, typename Dst, int TAPS>
__global__ __launch_bounds__(256) void to_output_rgb420_kernel(const Src* __restrict__ src, Dst* __restrict__ dst, int H, int W, ChromaTab tx, ChromaTab ty, PlanesRgb k)
{
    __shared__ int4 mid4[2 * RGB_SH * RGB_TW / 4];                                   // [2][RGB_SH][RGB_TW]: the row pass's sums of Cb, then of Cr
    __shared__ Src win[2 * RGB_SH * RGB_SW];                                         // [2][RGB_SH][RGB_SW]: the source windows
    int* const mid = (int*)mid4;
    const int h = H >> 1, w = W >> 1;
    const int X0 = blockIdx.x * RGB_TW, Y0 = blockIdx.y * RGB_TH;
    const int qx0 = (X0 >> 1) - RGB_LO, qy0 = (Y0 >> 1) - RGB_LO;
    const Src* const chroma = src + (long long)H * W;
    poly_window(chroma, h, w, qy0, qx0, win, RGB_SH, RGB_SW);
    poly_window(chroma + (long long)h * w, h, w, qy0, qx0, win + RGB_SH * RGB_SW, RGB_SH, RGB_SW);
    __syncthreads();
    {   // row pass: column X0 + (threadIdx.x & 127) of every window row of plane threadIdx.x >> 7 (columns past the frame's end read inside the window and are never used)
        const int col = threadIdx.x & (RGB_TW - 1), plane = threadIdx.x >> 7;
        const int X = X0 + col, q = X >> 1, p = X & 1;
        const Src* e = win + plane * RGB_SH * RGB_SW + q + tx.off[p] - qx0;
        int* const out = mid + plane * RGB_SH * RGB_TW + col;
        int c[TAPS];
        rgb_coefs(tx, p, c);
#pragma unroll 2
        for (int r = 0; r < RGB_SH; ++r) out[r * RGB_TW] = poly_dot24(c, e + r * RGB_SW, TAPS);
    }
    __syncthreads();
    // column pass and matrix: eight consecutive pixels of the two rows of one chroma row
    const int xs = (threadIdx.x & 15) * 8, qs = threadIdx.x >> 4;
    const int X = X0 + xs;
    if (X >= W) return;
    const int n = min(8, W - X);
    const bool rgb = k.rgb != 0, ordered = k.ordered != 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int Y = Y0 + 2 * qs + p;
        if (Y >= H) break;
        int c[TAPS], cb[8], cr[8], y[8];
        rgb_coefs(ty, p, c);
        const int* const m = mid + (qs + ty.off[p] + RGB_LO) * RGB_TW + xs;
        rgb_column8(c, m, k.cmax, cb);
        rgb_column8(c, m + RGB_SH * RGB_TW, k.cmax, cr);
        rgb_luma8(src + (long long)Y * W + X, n, y);
        StitchRun<Dst, 24> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int u = cb[e] - k.coff, v = cr[e] - k.coff;
            const long long base = (long long)k.coef[0] * (y[e] - k.yoff) + ((long long)quant_threshold(ordered, e, Y) << (RGB_FRAC - 7));      // (X is a multiple of 8: x & 7 = e)
            const Dst R = rgb_sample<Dst>(base + (long long)k.coef[1] * v, k.top);
            const Dst G = rgb_sample<Dst>(base + (long long)k.coef[2] * u + (long long)k.coef[3] * v, k.top);
            const Dst B = rgb_sample<Dst>(base + (long long)k.coef[4] * u, k.top);
            o.e[3 * e] = rgb ? R : B;
            o.e[3 * e + 1] = G;
            o.e[3 * e + 2] = rgb ? B : R;
        }
        stitch_store_n(dst + ((long long)Y * W + X) * 3, o, n);
    }
}

template <typename Src, typename Dst>
void launch_planes_rgb_t(const Src* src, int H, int W, Dst* dst, int taps, const ChromaTab& tx, const ChromaTab& ty, const PlanesRgb& k, hipStream_t s)
{
    const dim3 g((W + RGB_TW - 1) / RGB_TW, (H + RGB_TH - 1) / RGB_TH);
    if (taps == 1) hipLaunchKernelGGL((to_output_rgb420_kernel<Src, Dst, 1>), g, dim3(256), 0, s, src, dst, H, W, tx, ty, k);
    else if (taps == 2) hipLaunchKernelGGL((to_output_rgb420_kernel<Src, Dst, 2>), g, dim3(256), 0, s, src, dst, H, W, tx, ty, k);
    else hipLaunchKernelGGL((to_output_rgb420_kernel<Src, Dst, 4>), g, dim3(256), 0, s, src, dst, H, W, tx, ty, k);
}

}  // namespace

// Checked by moe_planes_to_rgb: H and W even and 2 at least, taps 1 / 2 / 4, the tables' sums and offsets, the constants' magnitudes.
void launch_planes_rgb(const void* src, int depth, int H, int W, void* dst, int bits, int taps, const ChromaTab& tx, const ChromaTab& ty, const PlanesRgb& k, hipStream_t s)
{
    poly_dispatch(src, depth, dst, bits == 8 ? 8 : 16, [&](auto* sp, auto* dp) { launch_planes_rgb_t(sp, H, W, dp, taps, tx, ty, k, s); });
}
