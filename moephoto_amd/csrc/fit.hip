// fit.hip -- planes of codes brought to a size that is no integer multiple of theirs (moe_fit_create / moe_fit_run; the definition: moephoto_amd/pixfmt.py, fitTable /
// fitPlanes): a rational n -> m integer polyphase filter per axis, stretched into an antialiasing filter where the axis shrinks, depth change included.  No floating
// point anywhere: the device's bytes are the definition's.
//
// Output index o reads the taps clamp(off[o] + j, 0, n - 1), j < T, with the 14-bit coefficients coef[o][j].  Every output index has a row of its own, so the tables
// live in device memory (uploaded once by moe_fit_create: per axis m offsets and m rows of FIT_TAPS coefficients, shorter rows ending in zeros; 8192 outputs are
// 288 KB, which stays in L2).  Row pass t = sum_j cx[o][j] * code in int32 (moe_fit_create refuses a row whose sum |c| * 65535 would not fit), column pass
// v = sum_i cy[o'][i] * t_i in int64, sample = clamp((v + 2^27) >> 28, 0, 2^Ds - 1) << (Dd - Ds) or >> (Ds - Dd).
//
// One workgroup of 256 threads = an output tile of FIT_TW x th samples of one plane (blockIdx.z); th is the host's choice (32, 16 or 8: the largest whose window fits
// the LDS budget).  The offsets do not decrease along an axis (checked at creation), so the tile's source window is [off[first], off[last] + T) per axis: it is read
// into LDS once, through clamped indices -- the edge sample repeats there and neither pass holds an edge case.  Row pass: one thread per tile column, its T
// coefficients in registers, every second window row -> int32 rows in LDS.  Column pass: one thread = eight consecutive samples of every sixteenth output row, the
// row's coefficients in registers, each run stored through stitch_store: 16 bytes at once where the address allows it -- the Cb plane starts wherever the Y plane
// ends.  T is a runtime value: the product loops are unrolled over FIT_TAPS with a uniform guard per tap (a scalar branch), so the coefficient registers are indexed by constants and nothing goes to scratch.
#include "common.h"
#include "run_store.h"

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
    const Src* const sp = src + (long long)blockIdx.z * h * w;
    for (int r = threadIdx.x >> 6; r < sh; r += 4) {
        const Src* row = sp + (long long)min(max(wy0 + r, 0), h - 1) * w;
        for (int c = threadIdx.x & 63; c < sw; c += 64) win[r * sw + c] = row[min(max(wx0 + c, 0), w - 1)];
    }
    __syncthreads();
    {   // row pass: tile column threadIdx.x & 127 (columns past the plane's end repeat the last one: computed inside the window, never stored)
        const int x = threadIdx.x & (FIT_TW - 1), X = min(X0 + x, X1);
        const int k0 = ax.off[X] - wx0, T = ax.taps;
        int c[FIT_TAPS];
        fit_coefs(ax.coef + (long long)X * FIT_TAPS, c);
        for (int r = threadIdx.x >> 7; r < sh; r += 2) {
            const Src* e = win + r * sw + k0;
            int t = 0;
#pragma unroll
            for (int j = 0; j < FIT_TAPS; ++j)
                if (j < T) t += __mul24(c[j], (int)e[j]);          // (|c| < 2^15, codes < 2^16: signed 24-bit factors; T is uniform: a scalar branch)
            mid[r * FIT_TW + x] = t;
        }
    }
    __syncthreads();
    const int xs = (threadIdx.x & 15) * 8, X = X0 + xs;
    if (X >= ow) return;
    Dst* const dp = dst + (long long)blockIdx.z * oh * ow;
    const int T = ay.taps;
#pragma unroll 1
    for (int Y = Y0 + (threadIdx.x >> 4); Y <= Y1; Y += 16) {
        const int* m = mid + (ay.off[Y] - wy0) * FIT_TW + xs;
        int c[FIT_TAPS];
        fit_coefs(ay.coef + (long long)Y * FIT_TAPS, c);
        long long v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 1ll << 27;
#pragma unroll
        for (int i = 0; i < FIT_TAPS; ++i) {
            if (i >= T) continue;
            const int4 a = *(const int4*)(m + i * FIT_TW), b = *(const int4*)(m + i * FIT_TW + 4);
            v[0] += (long long)c[i] * a.x; v[1] += (long long)c[i] * a.y; v[2] += (long long)c[i] * a.z; v[3] += (long long)c[i] * a.w;
            v[4] += (long long)c[i] * b.x; v[5] += (long long)c[i] * b.y; v[6] += (long long)c[i] * b.z; v[7] += (long long)c[i] * b.w;
        }
        StitchRun<Dst, 8> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int s = (int)min(max(v[e] >> 28, 0ll), (long long)smax);
            o.e[e] = (Dst)((s << shl) >> shr);
        }
        Dst* at = dp + (long long)Y * ow + X;
        if (X + 8 <= ow) stitch_store(at, o);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {      // (constant indices: a run indexed by a loop variable is moved to LDS)
                if (X + e >= ow) break;
                at[e] = o.e[e];
            }
        }
    }
}

template <typename Src, typename Dst>
void launch_fit_t(const void* src, int h, int w, void* dst, int oh, int ow, int planes, int th, size_t lds, const FitAxis& ax, const FitAxis& ay, int ds, int dd, hipStream_t s)
{
    const dim3 g((ow + FIT_TW - 1) / FIT_TW, (oh + th - 1) / th, planes);
    const int smax = (1 << ds) - 1, shl = dd > ds ? dd - ds : 0, shr = ds > dd ? ds - dd : 0;
    hipLaunchKernelGGL((resize_kernel_fit<Src, Dst>), g, dim3(256), lds, s, (const Src*)src, (Dst*)dst, h, w, oh, ow, th, ax, ay, smax, shl, shr);
}

}  // namespace

// src: `planes` planes of h x w codes at depth ds (uint8 for 8, else uint16); dst: as many planes of oh x ow at depth dd.  Checked by moe_fit_create: the tables' sums,
// offsets and order, th and lds (the LDS the largest window of a FIT_TW x th tile takes).
void launch_fit(const void* src, int ds, int h, int w, void* dst, int dd, int oh, int ow, int planes, int th, size_t lds, const FitAxis& ax, const FitAxis& ay, hipStream_t s)
{
    if (ds == 8) {
        if (dd == 8) launch_fit_t<uint8_t, uint8_t>(src, h, w, dst, oh, ow, planes, th, lds, ax, ay, ds, dd, s);
        else launch_fit_t<uint8_t, uint16_t>(src, h, w, dst, oh, ow, planes, th, lds, ax, ay, ds, dd, s);
    } else {
        if (dd == 8) launch_fit_t<uint16_t, uint8_t>(src, h, w, dst, oh, ow, planes, th, lds, ax, ay, ds, dd, s);
        else launch_fit_t<uint16_t, uint16_t>(src, h, w, dst, oh, ow, planes, th, lds, ax, ay, ds, dd, s);
    }
}
