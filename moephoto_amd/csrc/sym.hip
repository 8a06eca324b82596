// sym.hip -- the two passes of the SR self-ensemble around doCrop, python/imageProcess.py:563-572 and runSR.py:26 of the reference:
//
//     v = doCrop(x);  for i < n:  v = v + transInv[i](doCrop(opt, trans[i](x)));      sr: v / (n + 1)
//
// stitch_sym_pad_kernel    dst = padImage(trans_s(src)) in one pass: the symmetry and getPad's right / bottom padding (reflection with the edge not repeated, up to
//                          len - 1 samples, then zeros: python/imageProcess.py:47-56) are index arithmetic on a copy -- values are never converted
// stitch_sym_fold_kernel   acc <- acc + transInv_s(t) in place, in the canvas dtype as torch forms `v + view`: operands widened to fp32, added once, rounded once; the
//                          last fold also applies the closing `/ (n + 1)` to the freshly rounded sum, as torch's device kernel evaluates tensor / python_int: a
//                          multiplication by the fp32 reciprocal of the divisor (never fused with the sum: this file is compiled with -ffp-contract=off)
//
// Both are one index map (SymArgs, common.h): an axis of the destination maps to an axis of the source, reversed where the symmetry flips it.  Without a transpose a
// destination row is a source row: straight row copies.  With one, a 64 x 64 element tile goes through LDS: read along the source's rows, written along the
// destination's.  16-byte global loads and stores where base, pitch and run are 16-byte aligned, scalar ones elsewhere; every output element is written by exactly one
// thread; element offsets are 64-bit (a plane of a 32K canvas exceeds 2^31 bytes).
#include "common.h"

namespace {

// position k of a padded axis (n samples padded to np, k < np) -> the sample it shows (reversed: of the flipped axis), or -1 for a zero
__device__ __forceinline__ int sym_map(int k, int n, int np, int flip)
{
    if (k >= n) {
        const int r = k - n, refl = min(n - 1, np - n);
        if (r >= refl) return -1;
        k = n - 2 - r;
    }
    return flip ? n - 1 - k : k;
}

template <typename T> struct SymSum;
template <> struct SymSum<float> {
    static __device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
    static __device__ __forceinline__ float scale(float v, float inv) { return __fmul_rn(v, inv); }
};
template <> struct SymSum<half_t> {
    static __device__ __forceinline__ half_t add(half_t a, half_t b)
    {
#pragma clang fp contract(off)
        return (half_t)((float)a + (float)b);
    }
    // (half)((float)v * inv) with BOTH roundings, as torch's kernel has them: the product rounded to fp32 (v_mul_f32), then that to fp16 (v_cvt_f16_f32).  Left to
    // itself the compiler folds the pair into one v_fma_mixlo_f16 for some elements, which rounds the exact product ONCE: where the quotient is a subnormal tie the
    // bits differ -- a divisor of 6 separates the two forms on 342 of the 63,488 finite fp16 values (tests/test_gpu_sym.py goes through all of them).  The empty
    // asm keeps the product in its register between the two instructions.
    static __device__ __forceinline__ half_t scale(half_t v, float inv)
    {
        float p = __fmul_rn((float)v, inv);
        asm("" : "+v"(p));
        return (half_t)p;
    }
};

// VEC consecutive destination columns at dp: stored (pad) or folded into what is there (fold)
template <typename T, int VEC, bool FOLD>
__device__ __forceinline__ void sym_put(const SymArgs& a, T* dp, T (&val)[VEC])
{
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    if (FOLD) {
        const vec_t ov = *(const vec_t*)dp;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            val[k] = SymSum<T>::add(ov[k], val[k]);
            if (a.div) val[k] = SymSum<T>::scale(val[k], a.inv);
        }
    }
    vec_t o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = val[k];
    *(vec_t*)dp = o;
}

// no transpose: one thread = VEC consecutive columns of one destination row (VEC > 1: Wd is a multiple of it)
template <typename T, int VEC, bool FOLD>
__device__ __forceinline__ void sym_rows(const SymArgs& a)
{
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const int nv = a.Wd / VEC;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.C * a.Hd * nv) return;
    const int j = (int)(idx % nv) * VEC;
    const long long q = idx / nv;
    const int i = (int)(q % a.Hd), c = (int)(q / a.Hd);
    T val[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) val[k] = (T)0;
    const int sr = sym_map(i, a.nR, a.Hd, a.flipR);
    if (sr >= 0) {
        const T* sp = (const T*)a.src + c * a.sC + (long long)sr * a.sH;
        if (VEC > 1 && a.src_vec && j + VEC <= a.nC) {
            const vec_t sv = *(const vec_t*)(sp + (a.flipC ? a.nC - j - VEC : j));
#pragma unroll
            for (int k = 0; k < VEC; ++k) val[k] = a.flipC ? sv[VEC - 1 - k] : sv[k];
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int sc = sym_map(j + k, a.nC, a.Wd, a.flipC);
                if (sc >= 0) val[k] = sp[(long long)sc * a.sW];
            }
        }
    }
    sym_put<T, VEC, FOLD>(a, (T*)a.dst + ((long long)c * a.Hd + i) * a.Wd + j, val);
}

// transpose: one workgroup = one 64 x 64 tile of one destination plane.  tile[jj][ii] holds destination element (i0 + ii, j0 + jj): row jj is a piece of a SOURCE row.
// Row pitch 65 dwords (fp32) / 33 dwords (fp16): the transposed read -- lanes down a column -- finds every lane on a bank of its own.  With vectors a 32-lane half is
// 8 vectors x 4 rows on either side: 4 * 8 vector starts x 4 rows are 32 distinct banks in fp32; in fp16 the 8 vector starts of a column read fall on 4 banks, and rows
// 32.. of the tile are stored with their columns XOR 4 (two dwords further) to separate them.
template <typename T, int VEC, bool FOLD>
__device__ __forceinline__ void sym_tiles(const SymArgs& a)
{
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    constexpr int P = 64 + (sizeof(T) == 2 ? 2 : 1);
    constexpr int LPR = VEC == 1 ? 64 : 8;                 // lanes side by side along the contiguous axis
    constexpr int ITER = 64 * (64 / VEC) / 256;
    __shared__ T tile[64 * P];
    const int tw = (a.Wd + 63) / 64, th = (a.Hd + 63) / 64;
    long long b = blockIdx.x;
    const int j0 = (int)(b % tw) * 64;
    b /= tw;
    const int i0 = (int)(b % th) * 64, c = (int)(b / th);
    const T* sp = (const T*)a.src + c * a.sC;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int v = it * 256 + threadIdx.x;
        const int ii = ((v % LPR) + LPR * (v / (LPR * 64))) * VEC, jj = (v / LPR) % 64;
        const int i = i0 + ii, j = j0 + jj;
        T val[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) val[k] = (T)0;
        const int sr = j < a.Wd ? sym_map(j, a.nC, a.Wd, a.flipC) : -1;
        if (sr >= 0) {
            const T* rp = sp + (long long)sr * a.sH;
            if (VEC > 1 && a.src_vec && i + VEC <= a.nR) {
                const vec_t sv = *(const vec_t*)(rp + (a.flipR ? a.nR - i - VEC : i));
#pragma unroll
                for (int k = 0; k < VEC; ++k) val[k] = a.flipR ? sv[VEC - 1 - k] : sv[k];
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const int sc = i + k < a.Hd ? sym_map(i + k, a.nR, a.Hd, a.flipR) : -1;
                    if (sc >= 0) val[k] = rp[(long long)sc * a.sW];
                }
            }
        }
        const int sw = sizeof(T) == 2 ? (jj & 32) >> 3 : 0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) tile[jj * P + ((ii + k) ^ sw)] = val[k];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int v = it * 256 + threadIdx.x;
        const int jj = ((v % LPR) + LPR * (v / (LPR * 64))) * VEC, ii = (v / LPR) % 64;
        const int i = i0 + ii, j = j0 + jj;
        if (i >= a.Hd || j >= a.Wd) continue;              // (VEC > 1: Wd is a multiple of it -- a vector is inside or outside as a whole)
        T val[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int r = jj + k;
            val[k] = tile[r * P + (ii ^ (sizeof(T) == 2 ? (r & 32) >> 3 : 0))];
        }
        sym_put<T, VEC, FOLD>(a, (T*)a.dst + ((long long)c * a.Hd + i) * a.Wd + j, val);
    }
}

template <typename T, int VEC, bool TR>
__global__ __launch_bounds__(256) void stitch_sym_pad_kernel(SymArgs a)
{
    if (TR) sym_tiles<T, VEC, false>(a); else sym_rows<T, VEC, false>(a);
}

template <typename T, int VEC, bool TR>
__global__ __launch_bounds__(256) void stitch_sym_fold_kernel(SymArgs a)
{
    if (TR) sym_tiles<T, VEC, true>(a); else sym_rows<T, VEC, true>(a);
}

template <typename T, int VEC>
void launch_sym_as(const SymArgs& a, bool fold, bool tr, hipStream_t s)
{
    const long long tiles = (long long)a.C * ((a.Hd + 63) / 64) * ((a.Wd + 63) / 64);
    const long long rows = ((long long)a.C * a.Hd * (a.Wd / VEC) + 255) / 256;
    const dim3 g((unsigned)(tr ? tiles : rows)), b(256);
    if (fold) { if (tr) stitch_sym_fold_kernel<T, VEC, true><<<g, b, 0, s>>>(a); else stitch_sym_fold_kernel<T, VEC, false><<<g, b, 0, s>>>(a); }
    else { if (tr) stitch_sym_pad_kernel<T, VEC, true><<<g, b, 0, s>>>(a); else stitch_sym_pad_kernel<T, VEC, false><<<g, b, 0, s>>>(a); }
}

}  // namespace

void launch_sym(SymArgs a, bool f16, bool fold, bool tr, hipStream_t s)
{
    if (a.C <= 0 || a.Hd <= 0 || a.Wd <= 0) return;
    // vector stores: destination base and row pitch 16-byte aligned; vector loads: the same of the source, a unit column stride and -- where the axis is read
    // backwards -- a length that keeps the reversed runs on 16-byte boundaries
    const int V = f16 ? 8 : 4;
    const bool dst_vec = (uintptr_t)a.dst % 16 == 0 && a.Wd % V == 0;
    const int n_src = tr ? a.nR : a.nC, flip_src = tr ? a.flipR : a.flipC;
    a.src_vec = dst_vec && a.sW == 1 && (uintptr_t)a.src % 16 == 0 && a.sC % V == 0 && a.sH % V == 0 && (!flip_src || n_src % V == 0);
    if (f16) { if (dst_vec) launch_sym_as<half_t, 8>(a, fold, tr, s); else launch_sym_as<half_t, 1>(a, fold, tr, s); }
    else { if (dst_vec) launch_sym_as<float, 4>(a, fold, tr, s); else launch_sym_as<float, 1>(a, fold, tr, s); }
}
