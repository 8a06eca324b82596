// polyphase.h -- the arithmetic of the integer polyphase kernels, once: resize_kernel_codes (chroma.hip: integer scales, phase tables in the kernel's arguments),
// resize_kernel_fit (fit.hip: any n -> m, per-output tables in device memory) and resize_kernel_fit_px (fit_px.hip: the same on interleaved pixels).  The definition: moephoto_amd/pixfmt.py, _polyAxis / _polyPlanes.
// Output index o reads the taps clamp(first(o) + j, 0, n - 1) with 14-bit coefficients c[j] that sum to 2^14.  Row pass t = sum_j cx[j] * code in int32, column pass
// v = sum_i cy[i] * t_i in int64, sample = clamp((v + 2^27) >> 28, 0, 2^Ds - 1) << (Dd - Ds) or >> (Ds - Dd).  No floating point anywhere.
// A kernel keeps what is its own: the tile, where its window starts, where output o's first tap and coefficients come from, which thread computes which sample.
#pragma once
#include "common.h"
#include "run_store.h"

struct PolyQuant { int smax, shl, shr; };      // clamp to [0, smax = 2^Ds - 1], then << shl >> shr (one of the two is 0)

inline PolyQuant poly_quant(int ds, int dd) { return PolyQuant{(1 << ds) - 1, dd > ds ? dd - ds : 0, ds > dd ? ds - dd : 0}; }

// f(src, dst) with the pointers typed by the depths: uint8 samples at depth 8, else uint16
template <typename F>
void poly_dispatch(const void* src, int ds, void* dst, int dd, F f)
{
    if (ds == 8 && dd == 8) f((const uint8_t*)src, (uint8_t*)dst);
    else if (ds == 8) f((const uint8_t*)src, (uint16_t*)dst);
    else if (dd == 8) f((const uint16_t*)src, (uint8_t*)dst);
    else f((const uint16_t*)src, (uint16_t*)dst);
}

// The source window in LDS, win[sh][sw] = plane[clamp(y0 + r, 0, h - 1)][clamp(x0 + c, 0, w - 1)]: the edge sample repeats there and neither pass holds an edge case
// (the 256 threads of a workgroup: four rows at a time, 64 threads along a row)
template <typename Src>
__device__ __forceinline__ void poly_window(const Src* __restrict__ plane, int h, int w, int y0, int x0, Src* win, int sh, int sw)
{
    for (int r = threadIdx.x >> 6; r < sh; r += 4) {
        const Src* row = plane + (long long)min(max(y0 + r, 0), h - 1) * w;
        for (int c = threadIdx.x & 63; c < sw; c += 64) win[r * sw + c] = row[min(max(x0 + c, 0), w - 1)];
    }
}

// The same window of an interleaved image of C channels (fit_px.hip), x0 and sw counted in PIXELS: win[sh][sw * C], element c of a window row belongs to window
// pixel c / C and win[r][c] = image[clamp(y0 + r, 0, h - 1)][clamp(x0 + c / C, 0, w - 1)][c % C] -- the clamp is per pixel: past an edge the edge PIXEL repeats,
// channel by channel, where a clamp per element would repeat the last channel.
template <int C, typename Src>
__device__ __forceinline__ void poly_window_px(const Src* __restrict__ image, int h, int w, int y0, int x0, Src* win, int sh, int sw)
{
    // A thread's loads are issued in batches of up to KR rows x KC chunks of a row before the first of them is stored: with the few waves a CU holds beside a window of
    // this size, one load in flight per thread left the kernel waiting on memory latency (profiles/fit_px/summary.md).
    constexpr int KR = 4, KC = 4;
    const int n = sw * C;
    for (int r0 = threadIdx.x >> 6; r0 < sh; r0 += 4 * KR)
        for (int c0 = threadIdx.x & 63; c0 < n; c0 += 64 * KC) {
            Src v[KR][KC];
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                const Src* row = image + (long long)min(max(y0 + min(r0 + 4 * i, sh - 1), 0), h - 1) * w * C;      // (a row past the window reads the last one and is not stored)
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const int c = min(c0 + 64 * k, n - 1), p = c / C;                                              // (likewise a chunk past the row's end)
                    v[i][k] = row[min(max(x0 + p, 0), w - 1) * C + (c - p * C)];
                }
            }
#pragma unroll
            for (int i = 0; i < KR; ++i)
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (r0 + 4 * i < sh && c0 + 64 * k < n) win[(r0 + 4 * i) * n + c0 + 64 * k] = v[i][k];
        }
}

// sum_{j < taps} c[j] * e[j] in int32: |c| < 2^15 and codes < 2^16 are signed 24-bit factors, and the entry points refuse a row with sum |c| > 32767, so
// |t| <= 32767 * 65535 < 2^31.  taps is uniform: unrolled over N with a guard per tap (a scalar branch; a constant taps == N folds it away), so that c is indexed by
// constants -- a register array indexed by a runtime value goes to scratch.
template <int N, typename Src>
__device__ __forceinline__ int poly_dot24(const int (&c)[N], const Src* e, int taps)
{
    int t = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (j < taps) t += __mul24(c[j], (int)e[j]);
    return t;
}

// The column pass, the quantiser and the store of the first n of eight consecutive samples: v[e] = 2^27 + sum_{i < taps} c[i] * m[i * PITCH + e] in int64, where m points
// at the first tap's row of the row pass's sums (rows PITCH ints apart, m 16-byte aligned: two 16-byte LDS reads per tap) and 2^27 rounds the shift by 28.  The clamp
// is in 32 bits: |t| < 2^31 (above) and sum |c| <= 32767 again give |v| < 2^46 + 2^27, so v >> 28 fits an int for any uint16 code.
template <int PITCH, typename Dst, int N>
__device__ __forceinline__ void poly_run8(const int (&c)[N], const int* m, int taps, const PolyQuant& k, Dst* at, int n)
{
    long long v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 1ll << 27;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i >= taps) continue;
        const int4 a = *(const int4*)(m + i * PITCH), b = *(const int4*)(m + i * PITCH + 4);
        v[0] += (long long)c[i] * a.x; v[1] += (long long)c[i] * a.y; v[2] += (long long)c[i] * a.z; v[3] += (long long)c[i] * a.w;
        v[4] += (long long)c[i] * b.x; v[5] += (long long)c[i] * b.y; v[6] += (long long)c[i] * b.z; v[7] += (long long)c[i] * b.w;
    }
    StitchRun<Dst, 8> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int s = min(max((int)(v[e] >> 28), 0), k.smax);
        o.e[e] = (Dst)((s << k.shl) >> k.shr);
    }
    stitch_store_n(at, o, n);
}
