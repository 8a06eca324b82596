// fit_px.hip -- an INTERLEAVED image of codes (h x w pixels of C = 1 .. 4 channels: bgr24 / bgr48le frames, RGBA arrays) brought to a fitted size (moe_fit_create_px /
// moe_fit_run; the definition: moephoto_amd/pixfmt.py, fitPixels = fitPlanes on each channel).  fit.hip's kernel with one difference: a row of the image is a plane row of
// w * C ELEMENTS, and element e of an output row belongs to pixel e / C -- its offset and coefficients are that pixel's, and its tap j is the element C further on,
// window element (off + j) * C + e % C.  The column pass, the quantiser and the store see rows of ow * C elements and are polyphase.h's as they are.
//
// One workgroup of 256 threads = an output tile of FIT_TW ELEMENTS x th rows, whatever C is: the row pass keeps one thread per tile column and the column pass its runs
// of eight, so the int32 sums and the 16-byte stores are fit.hip's.  A tile edge may fall inside a pixel (C = 3: element 128 is channel 2 of pixel 42); nothing depends
// on it: the tile's window is that of the PIXELS its elements belong to, first to last, [off[X0 / C], off[X1 / C] + T) pixels, loaded whole -- poly_window_px clamps per
// pixel -- and each thread derives pixel and channel from its own element.  The host sized the LDS for the widest such window (moe_fit_create_px).
// LDS banks: neighbouring threads read neighbouring elements of the window (or, where the axis grows, the same ones: a broadcast); the tap stride C moves all of a
// wave's addresses alike, so the row pass's reads are as conflict-free as the planar kernel's at any C.
#include "polyphase.h"

namespace {

// the FIT_TAPS coefficients of one output index: fit.hip's fit_coefs word for word (two 16-byte loads, sign-extended into registers), kept here because fit.hip
// was not to change with this kernel -- both belong in polyphase.h, as one function, when fit.hip is next touched
__device__ __forceinline__ void fit_px_coefs(const short* __restrict__ row, int (&c)[FIT_TAPS])
{
    const int4 a = ((const int4*)row)[0], b = ((const int4*)row)[1];
    const int p[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[2 * k] = (p[k] << 16) >> 16;
        c[2 * k + 1] = p[k] >> 16;
    }
}

// poly_dot24 with the taps C elements apart: sum_{j < taps} c[j] * e[j * C], the same bound, the same uniform guard per tap
template <int C, int N, typename Src>
__device__ __forceinline__ int fit_px_dot24(const int (&c)[N], const Src* e, int taps)
{
    int t = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (j < taps) t += __mul24(c[j], (int)e[j * C]);
    return t;
}

// w / ow in pixels; owc = ow * C, the elements of an output row (checked by moe_fit_create_px to fit an int, as w * C)
template <typename Src, typename Dst, int C>
__global__ __launch_bounds__(256) void resize_kernel_fit_px(const Src* __restrict__ src, Dst* __restrict__ dst, int h, int w, int oh, int owc, int th, FitAxis ax, FitAxis ay,
                                                            int smax, int shl, int shr)
{
    extern __shared__ int4 fit_px_lds[];
    const int X0 = blockIdx.x * FIT_TW, Y0 = blockIdx.y * th;
    const int X1 = min(X0 + FIT_TW, owc) - 1, Y1 = min(Y0 + th, oh) - 1;          // the tile's last output element / row inside the image
    const int wx0 = ax.off[X0 / C], wy0 = ay.off[Y0];                             // the window starts at the first tap of the first element's PIXEL
    const int sw = ax.off[X1 / C] + ax.taps - wx0, sh = ay.off[Y1] + ay.taps - wy0;          // its extent in pixels / rows
    int* const mid = (int*)fit_px_lds;                       // [sh][FIT_TW]: the row pass's sums
    Src* const win = (Src*)(mid + sh * FIT_TW);              // [sh][sw * C]: the source window
    poly_window_px<C>(src, h, w, wy0, wx0, win, sh, sw);
    __syncthreads();
    {   // row pass: tile element threadIdx.x & 127 (elements past the row's end repeat the last one: computed inside the window, never stored), every second row
        const int x = threadIdx.x & (FIT_TW - 1), E = min(X0 + x, X1), P = E / C;
        const Src* e = win + (ax.off[P] - wx0) * C + (E - P * C);
        int c[FIT_TAPS];
        fit_px_coefs(ax.coef + (long long)P * FIT_TAPS, c);
        for (int r = threadIdx.x >> 7; r < sh; r += 2) mid[r * FIT_TW + x] = fit_px_dot24<C>(c, e + r * sw * C, ax.taps);
    }
    __syncthreads();
    // column pass: eight consecutive elements of every sixteenth row
    const int xs = (threadIdx.x & 15) * 8, X = X0 + xs;
    if (X >= owc) return;
#pragma unroll 1
    for (int Y = Y0 + (threadIdx.x >> 4); Y <= Y1; Y += 16) {
        int c[FIT_TAPS];
        fit_px_coefs(ay.coef + (long long)Y * FIT_TAPS, c);
        poly_run8<FIT_TW>(c, mid + (ay.off[Y] - wy0) * FIT_TW + xs, ay.taps, PolyQuant{smax, shl, shr}, dst + (long long)Y * owc + X, min(8, owc - X));
    }
}

template <int C>
void launch_fit_px_c(const void* src, int ds, int h, int w, void* dst, int dd, int oh, int ow, int th, size_t lds, const FitAxis& ax, const FitAxis& ay, hipStream_t s)
{
    const int owc = ow * C;
    const dim3 g((owc + FIT_TW - 1) / FIT_TW, (oh + th - 1) / th, 1);
    const PolyQuant k = poly_quant(ds, dd);
    poly_dispatch(src, ds, dst, dd, [&](auto* sp, auto* dp) {
        typedef std::remove_cv_t<std::remove_pointer_t<decltype(sp)>> S;
        typedef std::remove_pointer_t<decltype(dp)> D;
        hipLaunchKernelGGL((resize_kernel_fit_px<S, D, C>), g, dim3(256), lds, s, sp, dp, h, w, oh, owc, th, ax, ay, k.smax, k.shl, k.shr);
    });
}

}  // namespace

// src: h x w pixels of `channels` interleaved codes at depth ds (uint8 for 8, else uint16); dst: oh x ow pixels at depth dd.  Checked by moe_fit_create_px: channels
// (1 .. 4), the tables' sums, offsets and order, w * channels and ow * channels (ints), th and lds (the LDS the largest window of a tile of FIT_TW elements x th takes).
void launch_fit_px(const void* src, int ds, int h, int w, void* dst, int dd, int oh, int ow, int channels, int th, size_t lds, const FitAxis& ax, const FitAxis& ay, hipStream_t s)
{
    switch (channels) {
    case 1: launch_fit_px_c<1>(src, ds, h, w, dst, dd, oh, ow, th, lds, ax, ay, s); break;
    case 2: launch_fit_px_c<2>(src, ds, h, w, dst, dd, oh, ow, th, lds, ax, ay, s); break;
    case 3: launch_fit_px_c<3>(src, ds, h, w, dst, dd, oh, ow, th, lds, ax, ay, s); break;
    default: launch_fit_px_c<4>(src, ds, h, w, dst, dd, oh, ow, th, lds, ax, ay, s); break;
    }
}
