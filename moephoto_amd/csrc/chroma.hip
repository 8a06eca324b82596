// chroma.hip -- the chroma planes of a luma-only chain (moe_chroma_resample; the definition: moephoto_amd/pixfmt.py, chromaTable / resampleChroma): the Cb and Cr
// codes of a 4:2:0 frame brought to `scale` times their size by a fixed integer polyphase filter, depth change included.  No floating point anywhere: the device's
// bytes are the definition's.
//
// Output index o = q * scale + p reads the taps clamp(q + off[p] + j, 0, n - 1), j < TAPS, with the 14-bit coefficients coef[p][j]; both tables come from the caller
// (pixfmt.chromaTable) by value in the kernel's arguments, one per axis.  Row pass t = sum_j cx[p][j] * code in int32 (the entry point refuses a row whose
// sum |c| * 65535 would not fit), column pass v = sum_i cy[p'][i] * t_i in int64, sample = clamp((v + 2^27) >> 28, 0, 2^Ds - 1) << (Dd - Ds) or >> (Ds - Dd).
//
// One workgroup of 256 threads = an output tile of CHROMA_TW x CHROMA_TH samples of one plane (blockIdx.z).  Its source window -- the tile's source samples and
// CHROMA_LO before / CHROMA_HI behind them, what offsets in [-2, 1] and four taps can reach -- is read into LDS once, through clamped indices: the edge sample
// repeats there and neither pass holds an edge case.  Row pass: one thread per tile column (one division), every window row -> int32 rows in LDS.  Column pass: one
// thread = eight consecutive samples of four consecutive output rows (one division, then the phase counts up), each run stored through stitch_store: 16 bytes at
// once where the address allows it -- the Cb plane starts wherever the Y plane ends.  The kernel is bound by its stores: it writes scale^2 samples per sample read.
#include "common.h"
#include "run_store.h"

namespace {

constexpr int CHROMA_TW = 256, CHROMA_TH = 32;      // the output tile of a workgroup (tests/test_gpu_chroma.py derives its edge shapes from these)
constexpr int CHROMA_LO = 2, CHROMA_HI = 4;          // window margins: off >= -2;  off + TAPS - 1 <= 1 + 3

template <typename Src, typename Dst, int TAPS>
__global__ __launch_bounds__(256) void resize_kernel_codes(const Src* __restrict__ src, Dst* __restrict__ dst, int h, int w, int scale, int sw, int sh,
                                                           ChromaTab tx, ChromaTab ty, int smax, int shl, int shr)
{
    extern __shared__ int4 chroma_lds[];
    int* const mid = (int*)chroma_lds;                       // [sh][CHROMA_TW]: the row pass's sums
    Src* const win = (Src*)(mid + sh * CHROMA_TW);           // [sh][sw]: the source window
    const int OW = w * scale, OH = h * scale;
    const int X0 = blockIdx.x * CHROMA_TW, Y0 = blockIdx.y * CHROMA_TH;
    const int qx0 = X0 / scale - CHROMA_LO, qy0 = Y0 / scale - CHROMA_LO;
    const Src* const sp = src + (long long)blockIdx.z * h * w;
    for (int r = threadIdx.x >> 6; r < sh; r += 4) {
        const Src* row = sp + (long long)min(max(qy0 + r, 0), h - 1) * w;
        for (int c = threadIdx.x & 63; c < sw; c += 64) win[r * sw + c] = row[min(max(qx0 + c, 0), w - 1)];
    }
    __syncthreads();
    {   // row pass: column X0 + threadIdx.x of every window row (columns past the plane's end read inside the window and are never stored)
        const int X = X0 + threadIdx.x, q = X / scale, p = X - q * scale;
        const int k0 = q + tx.off[p] - qx0;
        int c[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; ++j) c[j] = tx.coef[p][j];
        for (int r = 0; r < sh; ++r) {
            const Src* e = win + r * sw + k0;
            int t = 0;
#pragma unroll
            for (int j = 0; j < TAPS; ++j) t += __mul24(c[j], (int)e[j]);          // (|c| < 2^15, codes < 2^16: signed 24-bit factors)
            mid[r * CHROMA_TW + threadIdx.x] = t;
        }
    }
    __syncthreads();
    const int xs = (threadIdx.x & 31) * 8, ys = (threadIdx.x >> 5) * 4;
    const int X = X0 + xs;
    if (X >= OW) return;
    Dst* const dp = dst + (long long)blockIdx.z * OH * OW;
    int Y = Y0 + ys, q = Y / scale, p = Y - q * scale;
#pragma unroll 1
    for (int n = 0; n < 4 && Y < OH; ++n, ++Y) {
        const int* m = mid + (q + ty.off[p] - qy0) * CHROMA_TW + xs;
        long long v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 1ll << 27;
#pragma unroll
        for (int i = 0; i < TAPS; ++i) {
            const int c = ty.coef[p][i];
            const int4 a = *(const int4*)(m + i * CHROMA_TW), b = *(const int4*)(m + i * CHROMA_TW + 4);
            v[0] += (long long)c * a.x; v[1] += (long long)c * a.y; v[2] += (long long)c * a.z; v[3] += (long long)c * a.w;
            v[4] += (long long)c * b.x; v[5] += (long long)c * b.y; v[6] += (long long)c * b.z; v[7] += (long long)c * b.w;
        }
        StitchRun<Dst, 8> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int s = min(max((int)(v[e] >> 28), 0), smax);
            o.e[e] = (Dst)((s << shl) >> shr);
        }
        Dst* at = dp + (long long)Y * OW + X;
        if (X + 8 <= OW) stitch_store(at, o);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {      // (constant indices: a run indexed by a loop variable is moved to LDS)
                if (X + e >= OW) break;
                at[e] = o.e[e];
            }
        }
        if (++p == scale) { p = 0; ++q; }
    }
}

template <typename Src, typename Dst>
void launch_chroma_t(const void* src, int h, int w, void* dst, int scale, int taps, const ChromaTab& tx, const ChromaTab& ty, int ds, int dd, hipStream_t s)
{
    // the window of a tile: at most (T - 1) / scale + 2 source samples under T output samples that start at any phase, and the margins
    const int sw = (CHROMA_TW - 1) / scale + 2 + CHROMA_LO + CHROMA_HI, sh = (CHROMA_TH - 1) / scale + 2 + CHROMA_LO + CHROMA_HI;
    const size_t lds = (size_t)sh * CHROMA_TW * sizeof(int) + (((size_t)sh * sw * sizeof(Src) + 15) & ~(size_t)15);          // 60.5 KB at scale 1, 17.5 KB at scale 4
    const dim3 g((w * scale + CHROMA_TW - 1) / CHROMA_TW, (h * scale + CHROMA_TH - 1) / CHROMA_TH, 2);
    const int smax = (1 << ds) - 1, shl = dd > ds ? dd - ds : 0, shr = ds > dd ? ds - dd : 0;
    const Src* sp = (const Src*)src;
    Dst* dp = (Dst*)dst;
    if (taps == 1) hipLaunchKernelGGL((resize_kernel_codes<Src, Dst, 1>), g, dim3(256), lds, s, sp, dp, h, w, scale, sw, sh, tx, ty, smax, shl, shr);
    else if (taps == 2) hipLaunchKernelGGL((resize_kernel_codes<Src, Dst, 2>), g, dim3(256), lds, s, sp, dp, h, w, scale, sw, sh, tx, ty, smax, shl, shr);
    else hipLaunchKernelGGL((resize_kernel_codes<Src, Dst, 4>), g, dim3(256), lds, s, sp, dp, h, w, scale, sw, sh, tx, ty, smax, shl, shr);
}

}  // namespace

// src: two planes of h x w codes at depth ds (uint8 for 8, else uint16); dst: two planes of h * scale x w * scale at depth dd.  Checked by moe_chroma_resample:
// scale 1 .. 16, taps 1 / 2 / 4, the tables' sums and offsets.
void launch_chroma_resample(const void* src, int ds, int h, int w, void* dst, int dd, int scale, int taps, const ChromaTab& tx, const ChromaTab& ty, hipStream_t s)
{
    if (ds == 8) {
        if (dd == 8) launch_chroma_t<uint8_t, uint8_t>(src, h, w, dst, scale, taps, tx, ty, ds, dd, s);
        else launch_chroma_t<uint8_t, uint16_t>(src, h, w, dst, scale, taps, tx, ty, ds, dd, s);
    } else {
        if (dd == 8) launch_chroma_t<uint16_t, uint8_t>(src, h, w, dst, scale, taps, tx, ty, ds, dd, s);
        else launch_chroma_t<uint16_t, uint16_t>(src, h, w, dst, scale, taps, tx, ty, ds, dd, s);
    }
}
