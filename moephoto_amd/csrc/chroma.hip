// chroma.hip -- the chroma planes of a luma-only chain (moe_chroma_resample; the definition: moephoto_amd/pixfmt.py, chromaTable / resampleChroma): the Cb and Cr
// codes of a 4:2:0 frame brought to `scale` times their size by a fixed integer polyphase filter, depth change included.  No floating point anywhere: the device's
// bytes are the definition's.
//
// Output index o = q * scale + p reads the taps clamp(q + off[p] + j, 0, n - 1), j < TAPS, with the 14-bit coefficients coef[p][j]; both tables come from the caller
// (pixfmt.chromaTable) by value in the kernel's arguments, one per axis.  The two passes, the quantiser and the store are polyphase.h's, shared with fit.hip.
//
// One workgroup of 256 threads = an output tile of CHROMA_TW x CHROMA_TH samples of one plane (blockIdx.z).  Its source window -- the tile's source samples and
// CHROMA_LO before / CHROMA_HI behind them, what offsets in [-2, 1] and four taps can reach -- is read into LDS once, through clamped indices: the edge sample
// repeats there and neither pass holds an edge case.  Row pass: one thread per tile column (one division), every window row -> int32 rows in LDS.  Column pass: one
// thread = eight consecutive samples of four consecutive output rows (one division, then the phase counts up), each run stored through stitch_store: 16 bytes at
// once where the address allows it -- the Cb plane starts wherever the Y plane ends.  The kernel is bound by its stores: it writes scale^2 samples per sample read.
#include "polyphase.h"

namespace {

constexpr int CHROMA_TW = 256, CHROMA_TH = 32;      // the output tile of a workgroup (tests/test_gpu_chroma.py derives its edge shapes from these)
constexpr int CHROMA_LO = 2, CHROMA_HI = 4;          // window margins: off >= -2;  off + TAPS - 1 <= 1 + 3

template <int TAPS>
__device__ __forceinline__ void chroma_coefs(const ChromaTab& t, int p, int (&c)[TAPS])
{
#pragma unroll
    for (int j = 0; j < TAPS; ++j) c[j] = t.coef[p][j];
}

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
    poly_window(src + (long long)blockIdx.z * h * w, h, w, qy0, qx0, win, sh, sw);
    __syncthreads();
    {   // row pass: column X0 + threadIdx.x of every window row (columns past the plane's end read inside the window and are never stored)
        const int X = X0 + threadIdx.x, q = X / scale, p = X - q * scale;
        const Src* e = win + q + tx.off[p] - qx0;
        int c[TAPS];
        chroma_coefs(tx, p, c);
        for (int r = 0; r < sh; ++r) mid[r * CHROMA_TW + threadIdx.x] = poly_dot24(c, e + r * sw, TAPS);
    }
    __syncthreads();
    // column pass: eight consecutive samples of four consecutive rows (one division, then the phase counts up)
    const int xs = (threadIdx.x & 31) * 8, ys = (threadIdx.x >> 5) * 4;
    const int X = X0 + xs;
    if (X >= OW) return;
    Dst* const dp = dst + (long long)blockIdx.z * OH * OW;
    int Y = Y0 + ys, q = Y / scale, p = Y - q * scale;
#pragma unroll 1
    for (int n = 0; n < 4 && Y < OH; ++n, ++Y) {
        int c[TAPS];
        chroma_coefs(ty, p, c);
        poly_run8<CHROMA_TW>(c, mid + (q + ty.off[p] - qy0) * CHROMA_TW + xs, TAPS, PolyQuant{smax, shl, shr}, dp + (long long)Y * OW + X, min(8, OW - X));
        if (++p == scale) { p = 0; ++q; }
    }
}

template <typename Src, typename Dst>
void launch_chroma_t(const Src* src, int h, int w, Dst* dst, int scale, int taps, const ChromaTab& tx, const ChromaTab& ty, PolyQuant k, hipStream_t s)
{
    // the window of a tile: at most (T - 1) / scale + 2 source samples under T output samples that start at any phase, and the margins
    const int sw = (CHROMA_TW - 1) / scale + 2 + CHROMA_LO + CHROMA_HI, sh = (CHROMA_TH - 1) / scale + 2 + CHROMA_LO + CHROMA_HI;
    const size_t lds = (size_t)sh * CHROMA_TW * sizeof(int) + (((size_t)sh * sw * sizeof(Src) + 15) & ~(size_t)15);          // 60.5 KB at scale 1, 17.5 KB at scale 4
    const dim3 g((w * scale + CHROMA_TW - 1) / CHROMA_TW, (h * scale + CHROMA_TH - 1) / CHROMA_TH, 2);
    if (taps == 1) hipLaunchKernelGGL((resize_kernel_codes<Src, Dst, 1>), g, dim3(256), lds, s, src, dst, h, w, scale, sw, sh, tx, ty, k.smax, k.shl, k.shr);
    else if (taps == 2) hipLaunchKernelGGL((resize_kernel_codes<Src, Dst, 2>), g, dim3(256), lds, s, src, dst, h, w, scale, sw, sh, tx, ty, k.smax, k.shl, k.shr);
    else hipLaunchKernelGGL((resize_kernel_codes<Src, Dst, 4>), g, dim3(256), lds, s, src, dst, h, w, scale, sw, sh, tx, ty, k.smax, k.shl, k.shr);
}

}  // namespace

// src: two planes of h x w codes at depth ds (uint8 for 8, else uint16); dst: two planes of h * scale x w * scale at depth dd.  Checked by moe_chroma_resample:
// scale 1 .. 16, taps 1 / 2 / 4, the tables' sums and offsets.
void launch_chroma_resample(const void* src, int ds, int h, int w, void* dst, int dd, int scale, int taps, const ChromaTab& tx, const ChromaTab& ty, hipStream_t s)
{
    poly_dispatch(src, ds, dst, dd, [&](auto* sp, auto* dp) { launch_chroma_t(sp, h, w, dp, scale, taps, tx, ty, poly_quant(ds, dd), s); });
}
