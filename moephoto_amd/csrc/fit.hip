// fit.hip -- planes of codes brought to a size that is no integer multiple of theirs (moe_fit_create / moe_fit_run; the definition: moephoto_amd/pixfmt.py, fitTable /
// fitPlanes): a rational n -> m integer polyphase filter per axis, stretched into an antialiasing filter where the axis shrinks, depth change included.  No floating
// point anywhere: the device's bytes are the definition's.
//
// Output index o reads the taps clamp(off[o] + j, 0, n - 1), j < T, with the 14-bit coefficients coef[o][j].  Every output index has a row of its own, so the tables
// live in device memory (uploaded once by moe_fit_create: per axis m offsets and m rows of FIT_TAPS coefficients, shorter rows ending in zeros; 8192 outputs are
// 288 KB, which stays in L2).  The two passes, the quantiser and the store are polyphase.h's, shared with chroma.hip.
//
// One workgroup of 256 threads = an output tile of FIT_TW x th samples of one plane (blockIdx.z); th is the host's choice (32, 16 or 8: the largest whose window fits
// the LDS budget).  The offsets do not decrease along an axis (checked at creation), so the tile's source window is [off[first], off[last] + T) per axis: it is read
// into LDS once, through clamped indices -- the edge sample repeats there and neither pass holds an edge case.  Row pass: one thread per tile column, its T
// coefficients in registers, every second window row -> int32 rows in LDS.  Column pass: one thread = eight consecutive samples of every sixteenth output row, the
// row's coefficients in registers, each run stored through stitch_store: 16 bytes at once where the address allows it -- the Cb plane starts wherever the Y plane
// ends.  T is a runtime value: the product loops are unrolled over FIT_TAPS with a uniform guard per tap (a scalar branch), so the coefficient registers are indexed by constants and nothing goes to scratch.
#include "polyphase.h"

namespace {

// the FIT_TAPS coefficients of one output index: two 16-byte loads (rows are 32 bytes, the table's base is 16-byte aligned), sign-extended into registers
__device__ __forceinline__ void fit_coefs(const short* __restrict__ row, int (&c)[FIT_TAPS])
{
    const int4 a = ((const int4*)row)[0], b = ((const int4*)row)[1];
    const int p[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[2 * k] = (p[k] << 16) >> 16;
        c[2 * k + 1] = p[k] >> 16;
    }
}

template <typename Src, typename Dst>
__global__ __launch_bounds__(256) void resize_kernel_fit(const Src* __restrict__ src, Dst* __restrict__ dst, int h, int w, int oh, int ow, int th, FitAxis ax, FitAxis ay,
                                                         int smax, int shl, int shr)
{
    extern __shared__ int4 fit_lds[];
    const int X0 = blockIdx.x * FIT_TW, Y0 = blockIdx.y * th;
    const int X1 = min(X0 + FIT_TW, ow) - 1, Y1 = min(Y0 + th, oh) - 1;          // the tile's last output column / row inside the plane
    const int wx0 = ax.off[X0], wy0 = ay.off[Y0];
    const int sw = ax.off[X1] + ax.taps - wx0, sh = ay.off[Y1] + ay.taps - wy0;          // the window's extent (the host sized the LDS for the largest of all tiles)
    int* const mid = (int*)fit_lds;                          // [sh][FIT_TW]: the row pass's sums
    Src* const win = (Src*)(mid + sh * FIT_TW);              // [sh][sw]: the source window
    poly_window(src + (long long)blockIdx.z * h * w, h, w, wy0, wx0, win, sh, sw);
    __syncthreads();
    {   // row pass: tile column threadIdx.x & 127 (columns past the plane's end repeat the last one: computed inside the window, never stored), every second row
        const int x = threadIdx.x & (FIT_TW - 1), X = min(X0 + x, X1);
        const Src* e = win + ax.off[X] - wx0;
        int c[FIT_TAPS];
        fit_coefs(ax.coef + (long long)X * FIT_TAPS, c);
        for (int r = threadIdx.x >> 7; r < sh; r += 2) mid[r * FIT_TW + x] = poly_dot24(c, e + r * sw, ax.taps);
    }
    __syncthreads();
    // column pass: eight consecutive samples of every sixteenth row
    const int xs = (threadIdx.x & 15) * 8, X = X0 + xs;
    if (X >= ow) return;
    Dst* const dp = dst + (long long)blockIdx.z * oh * ow;
#pragma unroll 1
    for (int Y = Y0 + (threadIdx.x >> 4); Y <= Y1; Y += 16) {
        int c[FIT_TAPS];
        fit_coefs(ay.coef + (long long)Y * FIT_TAPS, c);
        poly_run8<FIT_TW>(c, mid + (ay.off[Y] - wy0) * FIT_TW + xs, ay.taps, PolyQuant{smax, shl, shr}, dp + (long long)Y * ow + X, min(8, ow - X));
    }
}

}  // namespace

// src: `planes` planes of h x w codes at depth ds (uint8 for 8, else uint16); dst: as many planes of oh x ow at depth dd.  Checked by moe_fit_create: the tables' sums,
// offsets and order, th and lds (the LDS the largest window of a FIT_TW x th tile takes).
void launch_fit(const void* src, int ds, int h, int w, void* dst, int dd, int oh, int ow, int planes, int th, size_t lds, const FitAxis& ax, const FitAxis& ay, hipStream_t s)
{
    const dim3 g((ow + FIT_TW - 1) / FIT_TW, (oh + th - 1) / th, planes);
    const PolyQuant k = poly_quant(ds, dd);          // (passed as three ints: with the struct as the kernel's argument it measured 1 to 2 % slower, profiles/polyphase/summary.md)
    poly_dispatch(src, ds, dst, dd, [&](auto* sp, auto* dp) { hipLaunchKernelGGL(resize_kernel_fit, g, dim3(256), lds, s, sp, dp, h, w, oh, ow, th, ax, ay, k.smax, k.shl, k.shr); });
}
