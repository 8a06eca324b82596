// chroma_guided.hip -- the chroma planes of a luma-only chain, steered by the finished luma (moe_chroma_guided; the definition: moephoto_amd/pixfmt.py, guidedTable /
// lumaGuide / guidedChroma): a joint bilateral filter.  Every output chroma sample is a cubic B-spline over 4 x 4 source taps whose weights are multiplied by
// R[min(|GH - GL[tap]| >> 10, 63)], GH the OUTPUT frame's luma at the sample and GL the source frame's luma at the tap, both as 16-bit values at chroma resolution.
// Integers throughout and one exact division per sample and plane: the device's bytes are the definition's.
//
// One workgroup of 256 threads = an output tile of GUIDED_TW x GUIDED_TH chroma samples of BOTH planes: the weights of a sample are shared by Cb and Cr.  Its source
// window -- the tile's source samples and GUIDED_LO before / GUIDED_HI behind them, what offsets in [-2, 1] and four taps can reach -- is staged in LDS once, through
// clamped indices as polyphase.h's poly_window does (the edge sample repeats there and no tap holds an edge case), as one 8-byte entry per source sample:
// {Cb | Cr << 16, GL}, GL formed from the source frame's luma on the way in -- a tap is one 8-byte LDS read.  The phase tables and the range table lie in LDS too:
// they are indexed per lane.  One thread = eight consecutive samples of four consecutive output rows: it reads the two luma rows under its eight samples from the
// output frame (16-byte loads where the address allows them), forms GH, walks the 16 taps of each sample and stores the two runs through stitch_store: 16 bytes at
// once where the address allows it -- the Cb plane starts wherever the Y plane ends.
//
// The sums (the entry point checks what they rest on: 8-bit coefficient rows that sum to 256, range weights in 1 .. 255): a row of taps gives
// dr = sum_j cx[j] R_j <= 256 * 255 and nr = sum_j cx[j] R_j code_j <= 256 * 255 * 65535 < 2^32, both in 32 bits; den = sum_i cy[i] dr_i lies in [2^16, 2^24) and
// num = sum_i cy[i] nr_i < 2^40 in 64 bits.
#include "polyphase.h"

namespace {

constexpr int GUIDED_TW = 256, GUIDED_TH = 32;      // the output tile of a workgroup (tests/test_gpu_guided.py derives its edge shapes from these)
constexpr int GUIDED_LO = 2, GUIDED_HI = 4;          // window margins: off >= -2;  off + 3 <= 1 + 3

// s = floor((num + den / 2) / den), exactly, through one fp64 division: n = num + den / 2 < 2^41 and den < 2^24 are integers a double holds exactly, and the
// division is IEEE's (correctly rounded).  Where den divides n the quotient is an integer below 2^17 and comes out as it is.  Elsewhere the true quotient lies at
// least 1 / den > 2^-24 from the nearest integer, and its rounding moves it by at most half an ulp of a value below 2^17, 2^-37: it cannot reach that integer, and
// the truncation gives the floor.
__device__ __forceinline__ unsigned guided_divide(unsigned long long num, unsigned den)
{
    return (unsigned)((double)(num + (den >> 1)) / (double)den);
}

// v[k] += row[min(x + k, n - 1)], k < 16: sixteen consecutive luma samples of a row of n, the last one repeated past the row's end (those sums are never used).
// Whole 16-byte loads where all sixteen lie in the row and the address allows it.
template <typename T>
__device__ __forceinline__ void guided_luma16(const T* __restrict__ row, int x, int n, int (&v)[16])
{
    const T* p = row + x;
    if (x + 16 <= n && ((uintptr_t)p & 15) == 0) {
        if constexpr (sizeof(T) == 1) {
            const uint4 a = *(const uint4*)p;
            const unsigned q[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] += (q[k >> 2] >> (8 * (k & 3))) & 0xff;
        } else {
            const uint4 a = *(const uint4*)p, b = *(const uint4*)(p + 8);
            const unsigned q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] += (q[k >> 1] >> (16 * (k & 1))) & 0xffff;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] += (int)row[min(x + k, n - 1)];
    }
}

// The tables of a call, by value in the kernel's arguments: per phase the four 8-bit coefficients of an axis in one word (tap j in bits 8 j ..), the offsets, and the
// 64 range weights
struct GuidedTab { unsigned cx[16], cy[16]; signed char ox[16], oy[16]; unsigned char range[64]; };

template <typename Src, typename Dst>
__global__ __launch_bounds__(256) void resize_kernel_guided(const Src* __restrict__ src_c, const Src* __restrict__ src_y, Dst* __restrict__ dst_c,
                                                            const Dst* __restrict__ dst_y, int h, int w, int scale, int left, int sw, int sh, GuidedTab tab,
                                                            int gl_shl, int gh_shl, int shl, int shr)
{
    extern __shared__ int4 guided_lds[];
    unsigned* const t_cx = (unsigned*)guided_lds;                        // [16]
    unsigned* const t_cy = t_cx + 16;                                    // [16]
    signed char* const t_ox = (signed char*)(t_cy + 16);                 // [16]
    signed char* const t_oy = t_ox + 16;                                 // [16]
    unsigned char* const t_r = (unsigned char*)(t_oy + 16);              // [64]
    uint2* const win = (uint2*)(t_r + 64);                               // [sh][sw]: {Cb | Cr << 16, GL}; 224 bytes in, 8-byte aligned
    const int OW = w * scale, OH = h * scale;
    const int X0 = blockIdx.x * GUIDED_TW, Y0 = blockIdx.y * GUIDED_TH;
    const int qx0 = X0 / scale - GUIDED_LO, qy0 = Y0 / scale - GUIDED_LO;
    if (threadIdx.x < 16) {
        t_cx[threadIdx.x] = tab.cx[threadIdx.x];
        t_cy[threadIdx.x] = tab.cy[threadIdx.x];
        t_ox[threadIdx.x] = tab.ox[threadIdx.x];
        t_oy[threadIdx.x] = tab.oy[threadIdx.x];
    }
    if (threadIdx.x < 64) t_r[threadIdx.x] = tab.range[threadIdx.x];
    // the window: four rows at a time, 64 threads along a row (poly_window's walk); the luma block of a source sample is rows 2 y, 2 y + 1 and columns 2 x, 2 x + 1
    // ('center') or 2 x - 1, 2 x, 2 x + 1 with weights (1, 2, 1), the first clamped to the plane ('left'; 2 x + 1 is always inside)
    for (int r = threadIdx.x >> 6; r < sh; r += 4) {
        const int y = min(max(qy0 + r, 0), h - 1);
        const Src* const cb = src_c + (long long)y * w;
        const Src* const l0 = src_y + (long long)(2 * y) * (2 * w);
        const Src* const l1 = l0 + 2 * w;
        for (int c = threadIdx.x & 63; c < sw; c += 64) {
            const int x = min(max(qx0 + c, 0), w - 1);
            const int a = (int)l0[2 * x] + (int)l1[2 * x], b = (int)l0[2 * x + 1] + (int)l1[2 * x + 1];
            int g;
            if (left) {
                const int m = max(2 * x - 1, 0);
                g = (((int)l0[m] + (int)l1[m] + 2 * a + b) << gl_shl) >> 3;
            } else g = ((a + b) << gl_shl) >> 2;
            win[r * sw + c] = make_uint2((unsigned)cb[x] | (unsigned)cb[(long long)h * w + x] << 16, (unsigned)g);
        }
    }
    __syncthreads();
    const int xs = (threadIdx.x & 31) * 8, ys = (threadIdx.x >> 5) * 4;
    const int X = X0 + xs;
    if (X >= OW) return;
    const int qx = X / scale, px = X - qx * scale;
    const int LW = 2 * OW;                                               // the output frame's luma rows
    int Y = Y0 + ys, q = Y / scale, p = Y - q * scale;
#pragma unroll 1
    for (int n = 0; n < 4 && Y < OH; ++n, ++Y) {
        // GH of the eight samples: the sums of the two luma rows under them, then the block of each
        int v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0;
        const Dst* const l0 = dst_y + (long long)(2 * Y) * LW;
        guided_luma16(l0, 2 * X, LW, v);
        guided_luma16(l0 + LW, 2 * X, LW, v);
        int before = 0;
        if (left) {
            const int m = max(2 * X - 1, 0);
            before = (int)l0[m] + (int)l0[LW + m];
        }
        const unsigned cyw = t_cy[p];
        const uint2* const wrow = win + (q + t_oy[p] - qy0) * sw - qx0;
        int g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            g[e] = left ? (((e ? v[2 * e - 1] : before) + 2 * v[2 * e] + v[2 * e + 1]) << gh_shl) >> 3 : ((v[2 * e] + v[2 * e + 1]) << gh_shl) >> 2;
        // A loop that stays a loop: unrolled, the 128 LDS reads of a run are all issued first and their results fill the register file (256 VGPRs, one wave per
        // SIMD).  A register array indexed by the loop's variable would go to scratch, so the guides rotate through g[0] and the samples shift into two 64-bit
        // words per plane, 16 bits each: after eight turns sample e sits in bits 16 e .. of {lo, hi}.
        unsigned long long b_lo = 0, b_hi = 0, r_lo = 0, r_hi = 0;
        int xq = qx, xp = px;
#pragma unroll 1
        for (int e = 0; e < 8; ++e) {
            const int gh = g[0];
#pragma unroll
            for (int k = 0; k < 7; ++k) g[k] = g[k + 1];
            const unsigned cxw = t_cx[xp];
            const uint2* const tap = wrow + xq + t_ox[xp];
            unsigned den = 0;
            unsigned long long nb = 0, nr = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned dr = 0, rb = 0, rr = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint2 t = tap[i * sw + j];
                    const int d = gh - (int)t.y;
                    const unsigned k = ((cxw >> (8 * j)) & 0xff) * t_r[min((d < 0 ? -d : d) >> 10, 63)];
                    dr += k;
                    rb += k * (t.x & 0xffff);
                    rr += k * (t.x >> 16);
                }
                const unsigned c = (cyw >> (8 * i)) & 0xff;
                den += c * dr;
                nb += (unsigned long long)c * rb;
                nr += (unsigned long long)c * rr;
            }
            const unsigned long long sb = (guided_divide(nb, den) << shl) >> shr, sr = (guided_divide(nr, den) << shl) >> shr;
            b_lo = b_lo >> 16 | b_hi << 48;
            b_hi = b_hi >> 16 | sb << 48;
            r_lo = r_lo >> 16 | r_hi << 48;
            r_hi = r_hi >> 16 | sr << 48;
            if (++xp == scale) { xp = 0; ++xq; }
        }
        StitchRun<Dst, 8> ob, or_;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ob.e[e] = (Dst)((e < 4 ? b_lo : b_hi) >> (16 * (e & 3)));
            or_.e[e] = (Dst)((e < 4 ? r_lo : r_hi) >> (16 * (e & 3)));
        }
        Dst* const at = dst_c + (long long)Y * OW + X;
        const int run = min(8, OW - X);
        stitch_store_n(at, ob, run);
        stitch_store_n(at + (long long)OH * OW, or_, run);
        if (++p == scale) { p = 0; ++q; }
    }
}

template <typename Src, typename Dst>
void launch_guided_t(const Src* src_c, const Src* src_y, int ds, int h, int w, Dst* dst_c, const Dst* dst_y, int dd, int scale, int left, const GuidedTab& tab, hipStream_t s)
{
    // the window of a tile: at most (T - 1) / scale + 2 source samples under T output samples that start at any phase, and the margins
    const int sw = (GUIDED_TW - 1) / scale + 2 + GUIDED_LO + GUIDED_HI, sh = (GUIDED_TH - 1) / scale + 2 + GUIDED_LO + GUIDED_HI;
    const size_t lds = 224 + (size_t)sh * sw * sizeof(uint2);          // 24.5 KB at scale 2, 8.5 KB at scale 4
    const dim3 g((w * scale + GUIDED_TW - 1) / GUIDED_TW, (h * scale + GUIDED_TH - 1) / GUIDED_TH);
    hipLaunchKernelGGL((resize_kernel_guided<Src, Dst>), g, dim3(256), lds, s, src_c, src_y, dst_c, dst_y, h, w, scale, left, sw, sh, tab, 16 - ds, 16 - dd,
                       dd > ds ? dd - ds : 0, ds > dd ? ds - dd : 0);
}

}  // namespace

// src_c: two planes of h x w codes at depth ds, src_y: the 2 h x 2 w luma plane of the same frame; dst_c: two planes of h * scale x w * scale at depth dd, dst_y: the
// output frame's luma plane, 2 h * scale x 2 w * scale.  Checked by moe_chroma_guided: scale 2 .. 16, the tables' sums, offsets and range weights.
void launch_chroma_guided(const void* src_c, const void* src_y, int ds, int h, int w, void* dst_c, const void* dst_y, int dd, int scale, int left,
                          const unsigned char* cx, const signed char* ox, const unsigned char* cy, const signed char* oy, const unsigned char* range64, hipStream_t s)
{
    GuidedTab tab = {};
    for (int p = 0; p < scale; ++p) {
        for (int j = 0; j < 4; ++j) {
            tab.cx[p] |= (unsigned)cx[p * 4 + j] << (8 * j);
            tab.cy[p] |= (unsigned)cy[p * 4 + j] << (8 * j);
        }
        tab.ox[p] = ox[p];
        tab.oy[p] = oy[p];
    }
    for (int d = 0; d < 64; ++d) tab.range[d] = range64[d];
    poly_dispatch(src_c, ds, dst_c, dd, [&](auto* sp, auto* dp) {
        typedef std::remove_const_t<std::remove_pointer_t<decltype(sp)>> S;
        typedef std::remove_pointer_t<decltype(dp)> D;
        launch_guided_t((const S*)src_c, (const S*)src_y, ds, h, w, dp, (const D*)dst_y, dd, scale, left, tab, s);
    });
}
