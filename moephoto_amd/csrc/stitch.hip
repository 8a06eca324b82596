// stitch.hip -- the fold of the tile pool into the image (moe_stitch / moe_stitch_band, moe_stitch_out, moe_stitch_planes, moe_stitch_mix, moe_stitch_luma, moe_stitch_yuv): one skeleton, five edges on
// it and the Y'CbCr 4:2:0 edge over the same fold with a body of its own (chroma needs row pairs).
//
// Stitch: per-pixel fold of doCrop's sequential blend (imageProcess.py:120-131,167-170).  Every HR pixel visits,
// in raster tile order, the tiles whose written region covers it and applies
//     v1 = ex + wH*(r-ex)  (row inside the tile's blend band, else r);   v = ex + wW*(v1-ex)  (column likewise)
// with the same fp32 operation order as the reference, so the result is bit-identical to the sequential loop.
//
// What leaves the fold is the edge's business (an edge = a small policy type handed to stitch_fold):
//     CanvasEdge     the (C, rows, out_w) planes of the fp16 / fp32 canvas, or a band of its rows                                       stitch8r_kernel
//     SamplesEdge    the encoder's interleaved u8 / u16 samples: the canvas dtype's rounding and to_output_kernel's quantiser            stitch_out_kernel
//     PlaneEdge      the same samples at depth 8 / 10 / 12 / 16 as planes, one per blockIdx.z: the planes of a planar 4:2:0 frame            stitch_planes_kernel
//     MixEdge        the DN step: strengthOp's blend with the image the net saw and the alpha plane, in canvas or sample form            stitch_mix_kernel
//     LumaEdge       the merge of a luma-only step: Y' from the fold, Cb / Cr from two fp32 planes, the colour planes in canvas or sample form         stitch_luma_kernel
//     (YuvEdge)      the encoder's planar Y'CbCr 4:2:0 frame from SamplesEdge's 16-bit samples: half the bytes of the interleaved image      stitch_yuv_kernel
// The fold itself (stitch_classify, stitch_fold_row, stitch_pixel) exists once, so the bit equalities the tests demand between the edges (moe_stitch_out == moe_stitch ->
// float -> quantise, moe_stitch_mix == stitch + torch) hold by construction.  This file is compiled without extra flags: the fold's cur + w (q - cur) contracts to one FMA.
#include "common.h"
#include "run_store.h"
#include "luma.h"
#include "quant.h"
#include <type_traits>
#include "../../include/moephoto_amd.h"

namespace {

__device__ __forceinline__ float stitch_pixel(const StitchArgs& a, int X, int Y, int c)
{
    const int i0 = a.row_first[Y], ni = a.row_cnt[Y];
    const int j0 = a.col_first[X], nj = a.col_cnt[X];
    float cur = 0.f;
    for (int i = max(i0, a.row_lo); i < i0 + ni; ++i) {      // (row_lo: a band starts at the solid part of its first tile row, which overwrites whatever the rows above wrote)
        const int fy = a.row_tab[i * 4 + 0], sy = a.row_tab[i * 4 + 1], oy = a.row_tab[i * 4 + 2], eh = a.row_tab[i * 4 + 3];
        for (int j = j0; j < j0 + nj; ++j) {
            const int fx = a.col_tab[j * 4 + 0], sx = a.col_tab[j * 4 + 1], ox = a.col_tab[j * 4 + 2], ew = a.col_tab[j * 4 + 3];
            const float r = a.tiles[a.tile_off[i * a.step_w + j] + ((long long)c * eh + (Y - oy)) * ew + (X - ox)];
            float v1 = r;
            if (Y < sy) v1 = cur + a.ramp[Y - fy] * (r - cur);
            float v = v1;
            if (X < sx) v = cur + a.ramp[X - fx] * (v1 - cur);
            cur = v;
        }
    }
    return cur;
}

// The eight columns [X0, X0 + 8): true when they lie in the solid part of ONE tile column (k: that column, its origin and pitch) -- the vector path; false on a column
// seam and at the ragged end of a row (out_w % 8 != 0): those pixels go one by one through stitch_pixel.
struct StitchCols { int j0, ox, ew; };

__device__ __forceinline__ bool stitch_classify(const StitchArgs& a, int X0, StitchCols& k)
{
    if (!(X0 + 8 <= a.out_w)) return false;
    // every table entry is read before any is tested: four independent loads and one that depends on j0 (tested one by one with &&, each load waits for the test before it)
    const int j0 = a.col_first[X0], j7 = a.col_first[X0 + 7], n0 = a.col_cnt[X0], n7 = a.col_cnt[X0 + 7];
    const int sx = a.col_tab[j0 * 4 + 1];
    k.j0 = j0; k.ox = a.col_tab[j0 * 4 + 2]; k.ew = a.col_tab[j0 * 4 + 3];
    return (n0 == 1) & (n7 == 1) & (j7 == j0) & (X0 >= sx);
}

// Canvas row Y of the planes [c0, c0 + np), np <= NP, on the vector path: the covering tile rows in their order, per pixel the reference's cur = r, or
// cur + ramp (r - cur) inside the tile's blend band.  The row side (row tables, tile_off) is block-uniform and read once for all planes.
// (Returned by value: filled through a reference and read by the edge through another, the array left stitch_out_kernel<u16, 3, 4> with 140 VGPRs for 120.)
template <int NP> struct StitchFold { float v[NP][8]; };

template <int NP>
__device__ __forceinline__ StitchFold<NP> stitch_fold_row(const StitchArgs& a, const StitchCols& k, int X0, int Y, int c0, int np)
{
    StitchFold<NP> f;
    float (&cur)[NP][8] = f.v;
#pragma unroll
    for (int c = 0; c < NP; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) cur[c][e] = 0.f;
    const int i0 = a.row_first[Y], ni = a.row_cnt[Y];
    for (int i = max(i0, a.row_lo); i < i0 + ni; ++i) {
        const int fy = a.row_tab[i * 4 + 0], sy = a.row_tab[i * 4 + 1], oy = a.row_tab[i * 4 + 2], eh = a.row_tab[i * 4 + 3];
        const long long plane = (long long)eh * k.ew, o0 = a.tile_off[i * a.step_w + k.j0] + c0 * plane + (long long)(Y - oy) * k.ew + (X0 - k.ox);
        const bool band = Y < sy;
        const float wgt = band ? a.ramp[Y - fy] : 0.f;
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            if (c >= np) break;
            const long long t = o0 + c * plane;
            float q[8];
            if ((t & 3) == 0) {
                const float4 q0 = *(const float4*)(a.tiles + t), q1 = *(const float4*)(a.tiles + t + 4);
                q[0] = q0.x; q[1] = q0.y; q[2] = q0.z; q[3] = q0.w; q[4] = q1.x; q[5] = q1.y; q[6] = q1.z; q[7] = q1.w;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = a.tiles[t + e];
            }
            if (band) {
#pragma unroll
                for (int e = 0; e < 8; ++e) cur[c][e] = cur[c][e] + wgt * (q[e] - cur[c][e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) cur[c][e] = q[e];
            }
        }
    }
    return f;
}

// The skeleton: a block of 256 threads takes the canvas rows [Y0, Y0 + R) of [a.y0, a.y0 + a.rows) (a band: moe_stitch_band; the whole canvas: y0 = 0, rows = out_h)
// and 2048 columns; one thread = R rows x 8 consecutive pixels x the edge's NP planes.  An edge gives
//     NP, NOUT             planes a thread folds / elements it writes per pixel;   c0(), np(a): the planes [c0, c0 + np) it folds
//     Row                  what a thread holds of one row between fold and store
//     emit(a, X0, Y, cur, row)   fold -> Row;   store(a, X0, Y, row);   pixel(a, X, Y, c): one seam pixel's element c, folded with stitch_pixel and written
// History of this form on the 8K / 32K canvas (canvas edge): one pixel per thread 465 us; four pixels 350 us -- a chain of four dependent table loads per thread
// (col_first -> col_tab -> tile_off -> tile data) for 16 bytes of payload; eight pixels with a block-uniform row side
// 388 us / 4.46 ms = 1.6 / 2.1 TB/s; this form 1.88 ms on the 32K canvas = 5.1 TB/s.  What the last step removed: (1) a block lived for one
// chain of dependent loads and moved 12 KB with it -- now a block takes R rows, so one chain carries R x 2 independent 16-byte loads per
// thread; (2) seam ROWS (two covering tile rows: 4 % of the rows) sent every thread through the per-pixel fold -- now a thread whose eight
// columns lie in the solid part of ONE tile column folds the covering tile rows as vectors (stitch_fold_row); (3) a thread on a COLUMN seam
// walked its 8 pixels one after the other, ~5 dependent loads each, and held its wave meanwhile -- every fourth wave of a 2048-px tile
// column; now such threads only enlist their group and the whole block folds the seam pixels one pixel per thread.
template <int R, typename Edge>
__device__ __forceinline__ void stitch_fold(const StitchArgs& a, const Edge& edge)
{
    __shared__ int s_seam[256];
    __shared__ int s_nseam;
    if (threadIdx.x == 0) s_nseam = 0;
    __syncthreads();
    const int Y0 = blockIdx.y * R + a.y0, yend = a.y0 + a.rows;
    const int X0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (X0 < a.out_w) {
        StitchCols k;
        if (!stitch_classify(a, X0, k)) s_seam[atomicAdd(&s_nseam, 1)] = threadIdx.x;      // a column seam or the row's ragged end: handed to the whole block below
        else {
            typename Edge::Row o[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int Y = min(Y0 + r, yend - 1);               // (rows past the end repeat the last one and are not stored)
                const StitchFold<Edge::NP> f = stitch_fold_row<Edge::NP>(a, k, X0, Y, edge.c0(), edge.np(a));
                edge.emit(a, X0, Y, f.v, o[r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (Y0 + r >= yend) break;
                edge.store(a, X0, Y0 + r, o[r]);
            }
        }
    }
    __syncthreads();
    constexpr int PER = 8 * R * Edge::NOUT;      // elements of one enlisted group: (row, pixel, element), the element innermost
    const int total = s_nseam * PER;
    for (int t = threadIdx.x; t < total; t += 256) {
        const int gidx = t / PER, rem = t - gidx * PER;
        const int r = rem / (8 * Edge::NOUT), ec = rem - r * (8 * Edge::NOUT);
        const int e = ec / Edge::NOUT, c = ec - e * Edge::NOUT;
        const int X = (blockIdx.x * 256 + s_seam[gidx]) * 8 + e, Y = Y0 + r;
        if (Y >= yend || X >= a.out_w) continue;
        edge.pixel(a, X, Y, c);
    }
}

// ---------------------------------------------------------------------------------------------------
// The canvas (moe_stitch, moe_stitch_band): a.out = (C, rows, out_w) planes of half_t / float, one plane per blockIdx.z
// ---------------------------------------------------------------------------------------------------
struct CanvasEdge {
    static constexpr int NP = 1, NOUT = 1;
    struct Row { float v[8]; };
    __device__ __forceinline__ int c0() const { return blockIdx.z; }
    __device__ __forceinline__ int np(const StitchArgs&) const { return 1; }
    __device__ __forceinline__ long long at(const StitchArgs& a, int X, int Y) const { return ((long long)blockIdx.z * a.rows + (Y - a.y0)) * a.out_w + X; }
    __device__ __forceinline__ void emit(const StitchArgs&, int, int, const float (&cur)[1][8], Row& o) const
    {
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[e] = cur[0][e];
    }
    __device__ __forceinline__ void store(const StitchArgs& a, int X0, int Y, const Row& o) const
    {
        if (a.out_dtype == MOE_F16) {
            StitchRun<half_t, 8> h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h.e[e] = (half_t)o.v[e];
            stitch_store((half_t*)a.out + at(a, X0, Y), h);
        } else {
            StitchRun<float, 8> f;
#pragma unroll
            for (int e = 0; e < 8; ++e) f.e[e] = o.v[e];
            stitch_store((float*)a.out + at(a, X0, Y), f);
        }
    }
    __device__ __forceinline__ void pixel(const StitchArgs& a, int X, int Y, int) const
    {
        const float cur = stitch_pixel(a, X, Y, blockIdx.z);
        if (a.out_dtype == MOE_F16) ((half_t*)a.out)[at(a, X, Y)] = (half_t)cur;
        else ((float*)a.out)[at(a, X, Y)] = cur;
    }
};

template <int R>
__global__ __launch_bounds__(256) void stitch8r_kernel(StitchArgs a)
{
    stitch_fold<R>(a, CanvasEdge());
}

// ---------------------------------------------------------------------------------------------------
// Stitch straight into the encoder's bytes (moe_stitch_out): the fold, the rounding of the canvas dtype and to_output_kernel's quantiser in one pass -- the pool is
// read once and the interleaved u8 / u16 image written once; the fp16 / fp32 canvas and its fp32 copy (stitch -> toFloat -> toOutput: 17-18 bytes per pixel-plane) never
// exist.  The planes are inside the thread, so what it writes per row is one contiguous run of 8 * C elements.  Per element the operations of the three passes in
// their order, so the bytes are theirs.  (Times of this form and of the one-row-per-thread form before it, on the 8K frame beside the three passes:
// profiles/frame_stream/summary.md.)
// ---------------------------------------------------------------------------------------------------
// The quantiser is quant.h's quant_sample.  DITHER = true (the *_dither_kernel twins below, moe_stitch_out's MOE_Q_ROUND / MOE_Q_ORDERED): the rounding or ordered-dither
// form, at the pixel's coordinates in the image -- the vector path, the seam pass (pixel()) and the ragged row end hand the same (X, Y) to it.
template <typename TD, int C, bool DITHER = false>
struct SamplesEdge {
    static constexpr int NP = C, NOUT = C;
    typedef StitchRun<TD, 8 * C> Row;
    Quant<DITHER> q; bool f16;
    __device__ __forceinline__ int c0() const { return 0; }
    __device__ __forceinline__ int np(const StitchArgs&) const { return C; }
    __device__ __forceinline__ void emit(const StitchArgs&, int X0, int Y, const float (&cur)[C][8], Row& o) const
    {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) o.e[e * C + c] = quant_sample<TD>(cur[c][e], f16, q, X0 + e, Y);
    }
    __device__ __forceinline__ void store(const StitchArgs& a, int X0, int Y, const Row& o) const { stitch_store((TD*)a.out + ((long long)Y * a.out_w + X0) * C, o); }
    __device__ __forceinline__ void pixel(const StitchArgs& a, int X, int Y, int c) const
    {
        ((TD*)a.out)[((long long)Y * a.out_w + X) * C + c] = quant_sample<TD>(stitch_pixel(a, X, Y, c), f16, q, X, Y);
    }
};

template <typename TD, int C, int R>
__global__ __launch_bounds__(256) void stitch_out_kernel(StitchArgs a, float quant, int f16)
{
    stitch_fold<R>(a, SamplesEdge<TD, C>{{quant}, f16 != 0});
}

template <typename TD, int C, int R>
__global__ __launch_bounds__(256) void stitch_out_dither_kernel(StitchArgs a, QuantDither d, int f16)
{
    stitch_fold<R>(a, SamplesEdge<TD, C, true>{{d}, f16 != 0});
}

// ---------------------------------------------------------------------------------------------------
// The same samples as PLANES (moe_stitch_planes): a.out = a.C planes of out_h x out_w quantised samples at depth 8 (u8), 10, 12 or 16 (u16), plane c at
// a.out + c * out_h * out_w elements -- the Y' plane, or the Cb and Cr planes, of a planar 4:2:0 frame whose chain ran on the decoder's own planes (pixfmt.toPlanes /
// fromPlanes).  SamplesEdge's quantiser on CanvasEdge's layout: one plane per blockIdx.z, so a thread writes one run of eight samples per row.  The base is aligned
// only by luck (the Cb plane starts wherever the Y plane ends, inside a frame): every run goes through stitch_store.
// ---------------------------------------------------------------------------------------------------
template <typename TD, bool DITHER = false>
struct PlaneEdge {
    static constexpr int NP = 1, NOUT = 1;
    typedef StitchRun<TD, 8> Row;
    Quant<DITHER> q; bool f16;          // (DITHER: the thresholds at the sample's coordinates in its own plane)
    __device__ __forceinline__ int c0() const { return blockIdx.z; }
    __device__ __forceinline__ int np(const StitchArgs&) const { return 1; }
    __device__ __forceinline__ long long at(const StitchArgs& a, int X, int Y) const { return ((long long)blockIdx.z * a.out_h + Y) * a.out_w + X; }
    __device__ __forceinline__ void emit(const StitchArgs&, int X0, int Y, const float (&cur)[1][8], Row& o) const
    {
#pragma unroll
        for (int e = 0; e < 8; ++e) o.e[e] = quant_sample<TD>(cur[0][e], f16, q, X0 + e, Y);
    }
    __device__ __forceinline__ void store(const StitchArgs& a, int X0, int Y, const Row& o) const { stitch_store((TD*)a.out + at(a, X0, Y), o); }
    __device__ __forceinline__ void pixel(const StitchArgs& a, int X, int Y, int) const
    {
        ((TD*)a.out)[at(a, X, Y)] = quant_sample<TD>(stitch_pixel(a, X, Y, blockIdx.z), f16, q, X, Y);
    }
};

template <typename TD, int R>
__global__ __launch_bounds__(256) void stitch_planes_kernel(StitchArgs a, float quant, int f16)
{
    stitch_fold<R>(a, PlaneEdge<TD>{{quant}, f16 != 0});
}

template <typename TD, int R>
__global__ __launch_bounds__(256) void stitch_planes_dither_kernel(StitchArgs a, QuantDither d, int f16)
{
    stitch_fold<R>(a, PlaneEdge<TD, true>{{d}, f16 != 0});
}

// ---------------------------------------------------------------------------------------------------
// The DN step's edge in the stitch (moe_stitch_mix; plans of scale 1): RGBFilter's passes behind doCrop -- strengthOp's s * x + (1 - s) * inp and the alpha plane that
// rides around the net (python/imageProcess.py:350-377,562) -- inside the fold, and, in the sample form, toFloat / toOutput (:238-257) behind them.  Per
// pixel-plane, in T = the canvas dtype, as torch evaluates the expression on device tensors (scalars as fp32, every intermediate tensor in T):
//     c = T(fold);   y = T( T(sf * c) + T(tf * inp) );   strength 1: y = c (strengthOp returns x itself)
// The two products and the sum are three separately rounded fp32 operations: the empty asm statements keep each product in its register, so neither is fused into
// the sum (an FMA rounds once) nor, for fp16, into its own conversion (v_fma_mixlo_f16 rounds the exact product once; sym.hip's closing average met the same).  The
// fp32 sum of two fp16 values followed by its rounding to fp16 is the correctly rounded sum either way (24 >= 2 * 11 + 2 bits).
// Where torch itself rounds an fp16 product ONCE, so does this kernel (measured on torch 2.10, profiles/filter/summary.md): its vectorised elementwise kernel
// takes a dense tensor in blocks of 2048 elements and the last, partial block runs through other code, in which the compiler did pick v_fma_mixlo_f16 -- as it did in
// the kernel that serves strided views.  So element i of the (C, H, W) result has its products rounded once when i >= once_from = the start of that last block, and
// the input's product everywhere when the input is a view torch would not vectorise (m.q_once).  0.2 - 3 % of such elements differ by one fp16 ulp between the forms.
// A thread holds all CT output planes (R = 4, or 1 on small canvases: launch_stitch_mix_t).  Planes [0, a.C) are the net's; plane a.C (when CT > a.C) is alpha, copied.
// TD == T: the canvas form, dst = (CT, out_h, out_w) planes; else the sample form, dst = (out_h, out_w, CT) interleaved through to_output_kernel's quantiser.
// inp / alpha are read through element strides, as 16-byte vectors where m.inp_vec / m.alpha_vec say they may be.
// ---------------------------------------------------------------------------------------------------
// T(h * f): the product rounded to fp32, then to T
template <typename T>
__device__ __forceinline__ T stitch_mix_mul(T h, float f)
{
#pragma clang fp contract(off)
    float p = __fmul_rn(f, (float)h);
    asm("" : "+v"(p));
    return (T)p;
}

// fp16(h * f) with ONE rounding of the exact product: v_fma_mixlo_f16 with h read as fp16 from the low half of its register, f and the addend -0 as fp32
__device__ __forceinline__ half_t stitch_mix_mul_once(half_t h, float f)
{
    unsigned r;
    const unsigned hb = __builtin_bit_cast(unsigned short, h);
    const float nz = -0.0f;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hb), "v"(f), "v"(nz));
    return __builtin_bit_cast(half_t, (unsigned short)(r & 0xffffu));
}
__device__ __forceinline__ float stitch_mix_mul_once(float h, float f) { return stitch_mix_mul<float>(h, f); }      // (fp32: a product has one rounding anyway)

template <typename T>
__device__ __forceinline__ T stitch_mix_value(float cur, T inp, float sf, float tf, bool p_once, bool q_once)
{
#pragma clang fp contract(off)
    const T c = (T)cur;
    const T hp = p_once ? stitch_mix_mul_once(c, sf) : stitch_mix_mul<T>(c, sf);
    const T hq = q_once ? stitch_mix_mul_once(inp, tf) : stitch_mix_mul<T>(inp, tf);
    return (T)__fadd_rn((float)hp, (float)hq);
}

template <typename T>
__device__ __forceinline__ void stitch_mix_load8(const T* p, long long sW, bool vec, T (&v)[8])
{
    if (vec) {
        typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int N = 16 / sizeof(T);
#pragma unroll
        for (int k = 0; k < 8 / N; ++k) {
            const vec_t q = *(const vec_t*)(p + k * N);
#pragma unroll
            for (int e = 0; e < N; ++e) v[k * N + e] = q[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[e * sW];
    }
}

template <typename T, typename TD, int CT, bool DITHER = false>
struct MixEdge {
    static constexpr bool SAMPLE = !std::is_same<T, TD>::value;
    static constexpr int NP = CT, NOUT = CT;
    struct Planes { StitchRun<T, 8> p[CT]; };
    typedef typename std::conditional<SAMPLE, StitchRun<TD, 8 * CT>, Planes>::type Row;      // sample form: e[pixel * CT + plane]; canvas form: p[plane].e[pixel]
    const StitchMix& m;
    typename std::conditional<DITHER, QuantDither, QuantNone>::type d;          // the dithered sample form's quantiser (stitch_mix_dither_kernel); alpha is a channel of the pixel and shares its threshold
    template <typename V> __device__ __forceinline__ TD quant(V v, int X, int Y) const
    {
        if constexpr (DITHER) return quant_sample<TD, true>((float)v, false, d.S, d.top, d.ordered != 0, X, Y);
        else return quant_sample<TD, false>((float)v, false, m.quant, 0.f, false, X, Y);
    }
    __device__ __forceinline__ int c0() const { return 0; }
    __device__ __forceinline__ int np(const StitchArgs& a) const { return a.C; }
    __device__ __forceinline__ void emit(const StitchArgs& a, int X0, int Y, const float (&cur)[CT][8], Row& o) const
    {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            T y[8];
            if (c >= a.C) stitch_mix_load8((const T*)m.alpha + Y * m.aH + X0 * m.aW, m.aW, m.alpha_vec != 0, y);
            else if (m.blend) {
                const long long left = sizeof(T) == 2 ? m.once_from - (((long long)c * a.out_h + Y) * a.out_w + X0) : 8;      // elements of the run in front of once_from
                stitch_mix_load8((const T*)m.inp + c * m.sC + Y * m.sH + X0 * m.sW, m.sW, m.inp_vec != 0, y);
#pragma unroll
                for (int e = 0; e < 8; ++e) y[e] = stitch_mix_value<T>(cur[c][e], y[e], m.sf, m.tf, e >= left, e >= left || m.q_once);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) y[e] = (T)cur[c][e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if constexpr (SAMPLE) o.e[e * CT + c] = quant(y[e], X0 + e, Y);
                else o.p[c].e[e] = y[e];
            }
        }
    }
    __device__ __forceinline__ void store(const StitchArgs& a, int X0, int Y, const Row& o) const
    {
        if constexpr (SAMPLE) stitch_store((TD*)a.out + ((long long)Y * a.out_w + X0) * CT, o);
        else {
#pragma unroll
            for (int c = 0; c < CT; ++c) stitch_store((T*)a.out + ((long long)c * a.out_h + Y) * a.out_w + X0, o.p[c]);
        }
    }
    __device__ __forceinline__ void pixel(const StitchArgs& a, int X, int Y, int c) const
    {
        T y;
        if (c >= a.C) y = ((const T*)m.alpha)[Y * m.aH + X * m.aW];
        else {
            const float cur = stitch_pixel(a, X, Y, c);
            const bool p_once = sizeof(T) == 2 && ((long long)c * a.out_h + Y) * a.out_w + X >= m.once_from;
            y = m.blend ? stitch_mix_value<T>(cur, ((const T*)m.inp)[c * m.sC + Y * m.sH + X * m.sW], m.sf, m.tf, p_once, p_once || m.q_once) : (T)cur;
        }
        if constexpr (SAMPLE) ((TD*)a.out)[((long long)Y * a.out_w + X) * CT + c] = quant(y, X, Y);
        else ((T*)a.out)[((long long)c * a.out_h + Y) * a.out_w + X] = y;
    }
};

template <typename T, typename TD, int CT, int R>
__global__ __launch_bounds__(256) void stitch_mix_kernel(StitchArgs a, StitchMix m)
{
    stitch_fold<R>(a, MixEdge<T, TD, CT>{m});
}

template <typename T, typename TD, int CT, int R>
__global__ __launch_bounds__(256) void stitch_mix_dither_kernel(StitchArgs a, StitchMix m, QuantDither d)      // (the sample form only)
{
    stitch_fold<R>(a, MixEdge<T, TD, CT, true>{m, d});
}

// ---------------------------------------------------------------------------------------------------
// The merge of a luma-only step in the stitch (moe_stitch_luma; the definition: moephoto_amd/luma.py, the arithmetic: luma.h): the pool holds Y' alone (and alpha behind
// it when CT = 4), Cb / Cr come as two dense fp32 planes of the output's size, and the fold's edge writes the CT colour planes -- the Y' canvas never exists.  Per pixel
//     y = fp32(T(fold));   r = y + er cr;   b = y + eb cb;   g = y - (gr cr + gb cb);   each rounded to T;   alpha = T(fold of plane 1)
// exactly what moe_stitch -> moe_luma_merge give (to_output_luma_kernel runs the same luma.h functions).  A thread folds CT - 2 planes and holds CT output planes.
// TD == T: the canvas form, dst = (CT, out_h, out_w) planes; else the sample form, dst = (out_h, out_w, CT) interleaved through to_output_kernel's quantiser.
// The chroma runs are read as 16-byte vectors where their address allows it (out_w % 4 != 0 shifts every other row).
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TD, int CT, bool DITHER = false>
struct LumaEdge {
    static constexpr bool SAMPLE = !std::is_same<T, TD>::value;
    static constexpr int NP = CT - 2, NOUT = CT;
    struct Planes { StitchRun<T, 8> p[CT]; };
    typedef typename std::conditional<SAMPLE, StitchRun<TD, 8 * CT>, Planes>::type Row;      // sample form: e[pixel * CT + plane]; canvas form: p[plane].e[pixel]
    const StitchLuma& m;
    typename std::conditional<DITHER, QuantDither, QuantNone>::type d;          // the dithered sample form's quantiser (stitch_luma_dither_kernel)
    template <typename V> __device__ __forceinline__ TD quant(V v, int X, int Y) const
    {
        if constexpr (DITHER) return quant_sample<TD, true>((float)v, false, d.S, d.top, d.ordered != 0, X, Y);
        else return quant_sample<TD, false>((float)v, false, m.quant, 0.f, false, X, Y);
    }
    __device__ __forceinline__ int c0() const { return 0; }
    __device__ __forceinline__ int np(const StitchArgs&) const { return NP; }
    __device__ __forceinline__ void emit(const StitchArgs& a, int X0, int Y, const float (&cur)[NP][8], Row& o) const
    {
        const float* const pb = m.c + (long long)Y * a.out_w + X0;
        const float* const pr = pb + (long long)a.out_h * a.out_w;
        float cb[8], cr[8];
        stitch_mix_load8(pb, 1, ((uintptr_t)pb & 15) == 0, cb);
        stitch_mix_load8(pr, 1, ((uintptr_t)pr & 15) == 0, cr);
        T y[CT][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            luma_merge_planes<T>(m.k, (float)(T)cur[0][e], cb[e], cr[e], m.rp, y[0][e], y[1][e], y[2][e]);
            if constexpr (CT == 4) y[3][e] = luma_canon((T)cur[1][e]);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if constexpr (SAMPLE) o.e[e * CT + c] = quant(y[c][e], X0 + e, Y);
                else o.p[c].e[e] = y[c][e];
            }
    }
    __device__ __forceinline__ void store(const StitchArgs& a, int X0, int Y, const Row& o) const
    {
        if constexpr (SAMPLE) stitch_store((TD*)a.out + ((long long)Y * a.out_w + X0) * CT, o);
        else {
#pragma unroll
            for (int c = 0; c < CT; ++c) stitch_store((T*)a.out + ((long long)c * a.out_h + Y) * a.out_w + X0, o.p[c]);
        }
    }
    __device__ __forceinline__ void pixel(const StitchArgs& a, int X, int Y, int c) const
    {
        T y;
        if (c == 3) y = luma_canon((T)stitch_pixel(a, X, Y, 1));
        else {
            const long long at = (long long)Y * a.out_w + X;
            y = luma_canon((T)luma_merge_px(m.k, (float)(T)stitch_pixel(a, X, Y, 0), m.c[at], m.c[(long long)a.out_h * a.out_w + at], luma_colour(c, m.rp)));
        }
        if constexpr (SAMPLE) ((TD*)a.out)[((long long)Y * a.out_w + X) * CT + c] = quant(y, X, Y);
        else ((T*)a.out)[((long long)c * a.out_h + Y) * a.out_w + X] = y;
    }
};

template <typename T, typename TD, int CT, int R>
__global__ __launch_bounds__(256) void stitch_luma_kernel(StitchArgs a, StitchLuma m)
{
    stitch_fold<R>(a, LumaEdge<T, TD, CT>{m});
}

template <typename T, typename TD, int CT, int R>
__global__ __launch_bounds__(256) void stitch_luma_dither_kernel(StitchArgs a, StitchLuma m, QuantDither d)      // (the sample form only)
{
    stitch_fold<R>(a, LumaEdge<T, TD, CT, true>{m, d});
}

// ---------------------------------------------------------------------------------------------------
// The encoder's planar Y'CbCr 4:2:0 frame (moe_stitch_yuv, moe_to_yuv; the definition: moephoto_amd/pixfmt.py).  Per pixel the three planes are taken at 16 bits by
// SamplesEdge's quantiser -- the samples moe_stitch_out / moe_to_output write with bits = 16 -- and the conversion behind them is integer: Y per pixel, Cb and Cr from
// the sums of a 2 x 2 block.  The frame is 1.5 samples per pixel instead of 3: half the writes, half the download.
// stitch_yuv_kernel is the fold's fourth edge with a body of its own: the skeleton's hooks are per row and a chroma sample needs a row pair.  A vector-path thread
// owns 8 columns x R rows x 3 planes with X0 a multiple of 8 and Y0 a multiple of R (even), so no 2 x 2 block straddles two threads: it writes R runs of eight Y, R / 2
// runs of four Cb and of four Cr.  min(Y0 + r, out_h - 1) is the replication of the last row of an odd canvas.  Seam groups and the ragged row end go through the
// per-pixel fold one sample per thread, then one 2 x 2 block per thread; the odd last column is replicated there.  The Cb / Cr bases are aligned only by luck: every
// run goes through stitch_store.
// ---------------------------------------------------------------------------------------------------
// The dithered forms (stitch_yuv_dither_kernel, to_output_yuv_dither_kernel; the definition: quant.yuvFromSamples16): the 16-bit samples stay the truncating quantiser's and
// the two rounding constants become thresholds: 1 << (37 - D) -> T << (31 - D) and 1 << (39 - D) -> T << (33 - D).  Folded like the shifts: the luma numerator is scaled by
// 2^(D - 6) to reach >> 32, so T << (31 - D) becomes T << 25; the chroma numerator by 2^(D - 8) ((40 - D) + (D - 8) = 32), so T << (33 - D) becomes T << 25 as well.  T = 64
// ('round') is today's 2^31.  A chroma sample takes the threshold of its own coordinates in the chroma plane.
template <bool DITHER>
__device__ __forceinline__ unsigned yuv_round(bool ordered, int x, int y)
{
    if constexpr (DITHER) return quant_threshold(ordered, x, y) << 25;
    else return 0x80000000u;
}

__device__ __forceinline__ unsigned yuv_luma(const YuvEdge& y, unsigned p0, unsigned p1, unsigned p2, unsigned rnd = 0x80000000u)
{
    // < 2^30: the coefficients are positive and sum to 2^14.  24-bit multiplies (samples of 16 bits, coefficients of 14): v_mad_u32_u24 runs at the full rate, a
    // 32-bit v_mul_lo_u32 at a quarter of it -- with 32-bit products this edge was 216.9 us on the 8K canvas beside the sample edge's 203.1 (profiles/yuv/summary.md)
    const unsigned L = __umul24(y.ky[0], p0) + __umul24(y.ky[1], p1) + __umul24(y.ky[2], p2);
    return y.base_y + (unsigned)(((unsigned long long)L * y.mul_y + (unsigned long long)rnd) >> 32);             // one v_mad_u64_u32, its high word
}

// s0..s2: the planes' sums over the block, four samples each.  |M| <= 2^13 * 4 * 65535 < 2^31 whatever the order of the terms (the positive and the negative
// coefficients of a chroma row each sum to 2^13 in magnitude).
__device__ __forceinline__ unsigned yuv_chroma(const int (&k)[3], const YuvEdge& y, int s0, int s1, int s2, unsigned rnd = 0x80000000u)
{
    const int M = __mul24(k[0], s0) + __mul24(k[1], s1) + __mul24(k[2], s2);                             // (|k| <= 2^13, sums < 2^18: signed 24-bit factors)
    return (unsigned)(y.base_c + (int)(((long long)M * y.mul_c + (long long)rnd) >> 32));                 // (>> 32 of the signed sum: the floor shift of the definition)
}

__device__ __forceinline__ int yuv_sample16(float v, bool f16) { return quant_sample<uint16_t, false>(v, f16, 65536.f, 65536.f - 1.f, false, 0, 0); }

// (The body is stitch_yuv_body.inc, included by both kernels: see there.)
template <typename TD, int R>
__global__ __launch_bounds__(256) void stitch_yuv_kernel(StitchArgs a, YuvEdge y)
{
    constexpr bool DITHER = false;
    const bool ordered = false;
#include "stitch_yuv_body.inc"
}

template <typename TD, int R>
__global__ __launch_bounds__(256) void stitch_yuv_dither_kernel(StitchArgs a, YuvEdge y, int ordered_)
{
    constexpr bool DITHER = true;
    const bool ordered = ordered_ != 0;
#include "stitch_yuv_body.inc"
}

// The unfused form (moe_to_yuv): three dense planes of H x W -> the same frame, for chains whose last step is a resize, an ensemble or a blended DN.  One thread = one
// row pair x 8 columns; the samples are to_output_kernel's with bits = 16 (no canvas rounding: the planes are the canvas).
// (The body is to_output_yuv_body.inc, included by both kernels.)
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void to_output_yuv_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int H, int W, YuvEdge y)
{
    constexpr bool DITHER = false;
    const bool ordered = false;
#include "to_output_yuv_body.inc"
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void to_output_yuv_dither_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int H, int W, YuvEdge y, int ordered_)
{
    constexpr bool DITHER = true;
    const bool ordered = ordered_ != 0;
#include "to_output_yuv_body.inc"
}

}  // namespace

// One thread takes eight columns: any out_w, any base alignment, any number of tile columns.
void launch_stitch(const StitchArgs& a, hipStream_t s)
{
    if (a.rows <= 0) return;
    hipLaunchKernelGGL(stitch8r_kernel<4>, dim3(((a.out_w + 7) / 8 + 255) / 256, (a.rows + 3) / 4, a.C), dim3(256), 0, s, a);
}

template <typename TD>
static bool launch_stitch_out_t(const StitchArgs& a, float quant, int f16, hipStream_t s, const QuantDither* dq)
{
    constexpr int R = 4;          // rows per thread (the canvas edge's)
    const dim3 g(((a.out_w + 7) / 8 + 255) / 256, (a.rows + R - 1) / R);
    if (dq) {          // the rounding / ordered-dither quantiser: the same grid, the twin kernels
        if (a.C == 1) hipLaunchKernelGGL((stitch_out_dither_kernel<TD, 1, R>), g, dim3(256), 0, s, a, *dq, f16);
        else if (a.C == 2) hipLaunchKernelGGL((stitch_out_dither_kernel<TD, 2, R>), g, dim3(256), 0, s, a, *dq, f16);
        else if (a.C == 3) hipLaunchKernelGGL((stitch_out_dither_kernel<TD, 3, R>), g, dim3(256), 0, s, a, *dq, f16);
        else if (a.C == 4) hipLaunchKernelGGL((stitch_out_dither_kernel<TD, 4, R>), g, dim3(256), 0, s, a, *dq, f16);
        else return false;
        return true;
    }
    if (a.C == 1) hipLaunchKernelGGL((stitch_out_kernel<TD, 1, R>), g, dim3(256), 0, s, a, quant, f16);
    else if (a.C == 2) hipLaunchKernelGGL((stitch_out_kernel<TD, 2, R>), g, dim3(256), 0, s, a, quant, f16);
    else if (a.C == 3) hipLaunchKernelGGL((stitch_out_kernel<TD, 3, R>), g, dim3(256), 0, s, a, quant, f16);
    else if (a.C == 4) hipLaunchKernelGGL((stitch_out_kernel<TD, 4, R>), g, dim3(256), 0, s, a, quant, f16);
    else return false;
    return true;
}

// a.out: (out_h, out_w, C) interleaved, a.out_dtype MOE_U8 / MOE_U16; the whole canvas (y0 = 0, rows = out_h, row_lo = 0).  false: a plane count without a kernel
bool launch_stitch_out(const StitchArgs& a, int canvas_dtype, float quant, hipStream_t s, const QuantDither* dq)
{
    const int f16 = canvas_dtype == MOE_F16;
    return a.out_dtype == MOE_U8 ? launch_stitch_out_t<uint8_t>(a, quant, f16, s, dq) : launch_stitch_out_t<uint16_t>(a, quant, f16, s, dq);
}

template <typename TD>
static void launch_stitch_planes_t(const StitchArgs& a, float quant, int f16, hipStream_t s, const QuantDither* dq)
{
    // rows per thread: the sample edge's four, or one where four leave fewer than launch_stitch_mix_t's 1024 workgroups (a.C planes of them: blockIdx.z) -- the
    // chroma planes of a small frame
    const unsigned gx = ((a.out_w + 7) / 8 + 255) / 256;
    const bool four = (long long)gx * ((a.out_h + 3) / 4) * a.C >= 1024;
    if (dq) {
        if (four) hipLaunchKernelGGL((stitch_planes_dither_kernel<TD, 4>), dim3(gx, (a.out_h + 3) / 4, a.C), dim3(256), 0, s, a, *dq, f16);
        else hipLaunchKernelGGL((stitch_planes_dither_kernel<TD, 1>), dim3(gx, a.out_h, a.C), dim3(256), 0, s, a, *dq, f16);
    } else if (four) hipLaunchKernelGGL((stitch_planes_kernel<TD, 4>), dim3(gx, (a.out_h + 3) / 4, a.C), dim3(256), 0, s, a, quant, f16);
    else hipLaunchKernelGGL((stitch_planes_kernel<TD, 1>), dim3(gx, a.out_h, a.C), dim3(256), 0, s, a, quant, f16);
}

// a.out: a.C planes of out_h x out_w samples at `depth` bits, uint8 for depth 8, else uint16; the whole canvas (y0 = 0, rows = out_h, row_lo = 0)
void launch_stitch_planes(const StitchArgs& a, int canvas_dtype, int depth, hipStream_t s, const QuantDither* dq)
{
    const int f16 = canvas_dtype == MOE_F16;
    if (depth == 8) launch_stitch_planes_t<uint8_t>(a, 256.f, f16, s, dq);
    else launch_stitch_planes_t<uint16_t>(a, (float)(1 << depth), f16, s, dq);
}

template <typename T, typename TD, int R>
static bool launch_stitch_mix_r(const StitchArgs& a, const StitchMix& m, int planes, hipStream_t s, const QuantDither* dq)
{
    const dim3 g(((a.out_w + 7) / 8 + 255) / 256, (a.rows + R - 1) / R);
    if constexpr (!std::is_same<T, TD>::value) {
        if (dq) {
            if (planes == 1) hipLaunchKernelGGL((stitch_mix_dither_kernel<T, TD, 1, R>), g, dim3(256), 0, s, a, m, *dq);
            else if (planes == 2) hipLaunchKernelGGL((stitch_mix_dither_kernel<T, TD, 2, R>), g, dim3(256), 0, s, a, m, *dq);
            else if (planes == 3) hipLaunchKernelGGL((stitch_mix_dither_kernel<T, TD, 3, R>), g, dim3(256), 0, s, a, m, *dq);
            else if (planes == 4) hipLaunchKernelGGL((stitch_mix_dither_kernel<T, TD, 4, R>), g, dim3(256), 0, s, a, m, *dq);
            else return false;
            return true;
        }
    }
    if (planes == 1) hipLaunchKernelGGL((stitch_mix_kernel<T, TD, 1, R>), g, dim3(256), 0, s, a, m);
    else if (planes == 2) hipLaunchKernelGGL((stitch_mix_kernel<T, TD, 2, R>), g, dim3(256), 0, s, a, m);
    else if (planes == 3) hipLaunchKernelGGL((stitch_mix_kernel<T, TD, 3, R>), g, dim3(256), 0, s, a, m);
    else if (planes == 4) hipLaunchKernelGGL((stitch_mix_kernel<T, TD, 4, R>), g, dim3(256), 0, s, a, m);
    else return false;
    return true;
}

// Rows per thread: four where that still gives the device a few waves per SIMD (a 4K canvas and larger); one row on smaller canvases -- a DN
// step's 1080p frame is 270 workgroups of four rows on 256 CUs, one wave per SIMD waiting out its own loads (times of both: profiles/filter/summary.md).
template <typename T, typename TD>
static bool launch_stitch_mix_t(const StitchArgs& a, const StitchMix& m, int planes, hipStream_t s, const QuantDither* dq = nullptr)
{
    const long long blocks4 = (long long)(((a.out_w + 7) / 8 + 255) / 256) * ((a.out_h + 3) / 4);
    return blocks4 >= 1024 ? launch_stitch_mix_r<T, TD, 4>(a, m, planes, s, dq) : launch_stitch_mix_r<T, TD, 1>(a, m, planes, s, dq);
}

// a.C: the net's planes; with m.alpha one more plane is written.  m.quant == 0: a.out = the canvas (planes, out_h, out_w) of canvas_dtype; else a.out = interleaved
// (out_h, out_w, planes) of a.out_dtype MOE_U8 / MOE_U16.  The whole canvas (y0 = 0, rows = out_h, row_lo = 0).  false: a plane count without a kernel
bool launch_stitch_mix(const StitchArgs& a, StitchMix m, int canvas_dtype, hipStream_t s, const QuantDither* dq)
{
    const int planes = a.C + (m.alpha ? 1 : 0);
    const bool f16 = canvas_dtype == MOE_F16;
    const long long V = f16 ? 8 : 4;          // elements of a 16-byte vector: base, plane and row pitch must be multiples of it
    m.inp_vec = m.sW == 1 && (uintptr_t)m.inp % 16 == 0 && m.sC % V == 0 && m.sH % V == 0;
    m.alpha_vec = m.alpha && m.aW == 1 && (uintptr_t)m.alpha % 16 == 0 && m.aH % V == 0;
    // where torch rounds an fp16 product once (MixEdge's comment): from the last, partial block of 2048 elements of the dense (C, H, W) result on; the input's
    // product everywhere unless the input has a unit column stride and a 16-byte aligned base -- the image itself or its padded copy, which torch sees as a dense tensor
    m.once_from = (long long)a.C * a.out_h * a.out_w / 2048 * 2048;
    m.q_once = f16 && !(m.sW == 1 && (uintptr_t)m.inp % 16 == 0);
    if (m.quant == 0.f) return f16 ? launch_stitch_mix_t<half_t, half_t>(a, m, planes, s) : launch_stitch_mix_t<float, float>(a, m, planes, s);
    if (a.out_dtype == MOE_U8) return f16 ? launch_stitch_mix_t<half_t, uint8_t>(a, m, planes, s, dq) : launch_stitch_mix_t<float, uint8_t>(a, m, planes, s, dq);
    return f16 ? launch_stitch_mix_t<half_t, uint16_t>(a, m, planes, s, dq) : launch_stitch_mix_t<float, uint16_t>(a, m, planes, s, dq);
}

template <typename T, typename TD, int R>
static bool launch_stitch_luma_r(const StitchArgs& a, const StitchLuma& m, hipStream_t s, const QuantDither* dq)
{
    const dim3 g(((a.out_w + 7) / 8 + 255) / 256, (a.rows + R - 1) / R);
    if constexpr (!std::is_same<T, TD>::value) {
        if (dq) {
            if (a.C == 1) hipLaunchKernelGGL((stitch_luma_dither_kernel<T, TD, 3, R>), g, dim3(256), 0, s, a, m, *dq);
            else if (a.C == 2) hipLaunchKernelGGL((stitch_luma_dither_kernel<T, TD, 4, R>), g, dim3(256), 0, s, a, m, *dq);
            else return false;
            return true;
        }
    }
    if (a.C == 1) hipLaunchKernelGGL((stitch_luma_kernel<T, TD, 3, R>), g, dim3(256), 0, s, a, m);
    else if (a.C == 2) hipLaunchKernelGGL((stitch_luma_kernel<T, TD, 4, R>), g, dim3(256), 0, s, a, m);
    else return false;
    return true;
}

template <typename T, typename TD>
static bool launch_stitch_luma_t(const StitchArgs& a, const StitchLuma& m, hipStream_t s, const QuantDither* dq = nullptr)      // (rows per thread: launch_stitch_mix_t's rule)
{
    const long long blocks4 = (long long)(((a.out_w + 7) / 8 + 255) / 256) * ((a.out_h + 3) / 4);
    return blocks4 >= 1024 ? launch_stitch_luma_r<T, TD, 4>(a, m, s, dq) : launch_stitch_luma_r<T, TD, 1>(a, m, s, dq);
}

// a.C: the pool's planes, 1 (Y') or 2 (Y', alpha); a.C + 2 planes are written.  m.quant == 0: a.out = the canvas (a.C + 2, out_h, out_w) of canvas_dtype; else a.out =
// interleaved (out_h, out_w, a.C + 2) of a.out_dtype MOE_U8 / MOE_U16.  The whole canvas (y0 = 0, rows = out_h, row_lo = 0).  false: a plane count without a kernel
bool launch_stitch_luma(const StitchArgs& a, const StitchLuma& m, int canvas_dtype, hipStream_t s, const QuantDither* dq)
{
    const bool f16 = canvas_dtype == MOE_F16;
    if (m.quant == 0.f) return f16 ? launch_stitch_luma_t<half_t, half_t>(a, m, s) : launch_stitch_luma_t<float, float>(a, m, s);
    if (a.out_dtype == MOE_U8) return f16 ? launch_stitch_luma_t<half_t, uint8_t>(a, m, s, dq) : launch_stitch_luma_t<float, uint8_t>(a, m, s, dq);
    return f16 ? launch_stitch_luma_t<half_t, uint16_t>(a, m, s, dq) : launch_stitch_luma_t<float, uint16_t>(a, m, s, dq);
}

// a.out: the Y'CbCr 4:2:0 frame of a.out_h x a.out_w (uint8 for depth 8, else uint16); three planes, the whole canvas (y0 = 0, rows = out_h, row_lo = 0)
void launch_stitch_yuv(const StitchArgs& a, const YuvEdge& y, hipStream_t s, int dither)
{
    constexpr int R = 4;          // rows per thread (the sample edge's): two chroma rows
    const dim3 g(((a.out_w + 7) / 8 + 255) / 256, (a.out_h + R - 1) / R);
    if (dither) {
        const int ordered = dither == 2;
        if (y.depth == 8) hipLaunchKernelGGL((stitch_yuv_dither_kernel<uint8_t, R>), g, dim3(256), 0, s, a, y, ordered);
        else hipLaunchKernelGGL((stitch_yuv_dither_kernel<uint16_t, R>), g, dim3(256), 0, s, a, y, ordered);
    } else if (y.depth == 8) hipLaunchKernelGGL((stitch_yuv_kernel<uint8_t, R>), g, dim3(256), 0, s, a, y);
    else hipLaunchKernelGGL((stitch_yuv_kernel<uint16_t, R>), g, dim3(256), 0, s, a, y);
}

void launch_to_output_yuv(const void* src, int src_dtype, int H, int W, const YuvEdge& y, void* dst, hipStream_t s, int dither)
{
    const dim3 g(((W + 7) / 8 + 255) / 256, (H + 1) / 2);
    if (dither) {
        const int ordered = dither == 2;
        if (src_dtype == MOE_F16) {
            if (y.depth == 8) hipLaunchKernelGGL((to_output_yuv_dither_kernel<half_t, uint8_t>), g, dim3(256), 0, s, (const half_t*)src, (uint8_t*)dst, H, W, y, ordered);
            else hipLaunchKernelGGL((to_output_yuv_dither_kernel<half_t, uint16_t>), g, dim3(256), 0, s, (const half_t*)src, (uint16_t*)dst, H, W, y, ordered);
        } else {
            if (y.depth == 8) hipLaunchKernelGGL((to_output_yuv_dither_kernel<float, uint8_t>), g, dim3(256), 0, s, (const float*)src, (uint8_t*)dst, H, W, y, ordered);
            else hipLaunchKernelGGL((to_output_yuv_dither_kernel<float, uint16_t>), g, dim3(256), 0, s, (const float*)src, (uint16_t*)dst, H, W, y, ordered);
        }
    } else if (src_dtype == MOE_F16) {
        if (y.depth == 8) hipLaunchKernelGGL((to_output_yuv_kernel<half_t, uint8_t>), g, dim3(256), 0, s, (const half_t*)src, (uint8_t*)dst, H, W, y);
        else hipLaunchKernelGGL((to_output_yuv_kernel<half_t, uint16_t>), g, dim3(256), 0, s, (const half_t*)src, (uint16_t*)dst, H, W, y);
    } else {
        if (y.depth == 8) hipLaunchKernelGGL((to_output_yuv_kernel<float, uint8_t>), g, dim3(256), 0, s, (const float*)src, (uint8_t*)dst, H, W, y);
        else hipLaunchKernelGGL((to_output_yuv_kernel<float, uint16_t>), g, dim3(256), 0, s, (const float*)src, (uint16_t*)dst, H, W, y);
    }
}
