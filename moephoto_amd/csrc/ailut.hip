// ailut.hip -- the AiLUT generator net (moe_ailut_run; the definition: moephoto_amd/ailut.py, thumbnail / generate): the small net of the reference's "Retouch" that
// looks at a 256 x 256 thumbnail of the frame and writes the frame's own 3D table and vertices (python/AiLUT.py:26-46 TPAMIBackbone with extra_pooling, :57-80
// LUTGenerator, :82-121 AdaInt, :167-181 AiLUT.forward up to ailut_transform) into a moe_lut3d handle's device layout, in front of lut3d.hip's launch.
//
// About 150 MFLOP per frame on a fixed 256 x 256 input: every launch is short and bound by latency, not by a pipe.  Parameters and activations are fp32 (the
// reference runs the net under fp16 autocast; the table multiplies into every pixel, so this does not); every dot product is accumulated by plain VALU FMAs in
// fp64, where a product of two fp32 values is exact, and rounded to fp32 ONCE, behind bias and activation.  Why not fp32 accumulators: on a flat frame a map is one
// constant c inside a border, so var is a few per cent of c^2 and the norm scales every absolute error of its input by rstd ~ 6 / |c|; an fp32 sum of n terms
// carries up to n 2^-24 |c| where the one storage rounding carries 2^-24 |c|, and the parity bound -- four times the error of ONE other fp32 implementation on the
// same frame -- leaves no room for a summation order that happens to be a few times worse than that implementation's (profiles/ailut/parity.md).  At these sizes
// the fp64 rate costs nothing that the launches' latency does not hide.  One launch per layer, ordered by the stream: the thumbnail, five conv blocks, the heads,
// the table.  No cooperative launch, no grid-wide barrier, no atomics of any kind: every word of every buffer is written by exactly one thread of
// exactly one workgroup on every run, and every sum has a fixed order, so two runs on the same input give the same bits and nothing of an earlier frame survives.
//
// A conv block is Conv2d(3 x 3, stride 2, padding 1) -> LeakyReLU(0.2) [-> InstanceNorm].  The block's kernel writes the activation BEFORE the norm and, per
// workgroup, the partial (sum, sum of squares) of each of its channels as DOUBLES (a thread's fp32 value widened, a fixed butterfly over the wave, a fixed order
// over the workgroup's waves).  The consumer reduces a channel's partials in a fixed order, in fp64: mean = S / N, var = max(Q / N - mean^2, 0) -- with 53 bits the
// cancellation costs (mean^2 / var) 2^-53 relative, beside fp32 activations nothing -- and applies (x - mean) (rstd gamma) + beta in fp64 as it loads.  Zero
// padding applies after the affine: an out-of-range tap contributes 0, not beta.
//
// Filling the device: a wave owns 64 output pixels and CO_T output channels, so that the weights are wave-uniform (scalar loads).  The
// workgroup's four waves are either four pixel groups (KS = 1: the wide early layers) or KS slices of the input channels of the same pixels (layers 2 .. 5, whose
// 288- to 1 152-term dot products would otherwise leave a thread a long serial loop and the device a few dozen workgroups): the slices meet in LDS and wave 0 adds
// them in slice order.  256 workgroups for layers 1 .. 4, 128 for layer 5.
#include "common.h"

namespace {

constexpr int TS = AILUT_SIZE;
constexpr double AILUT_SLOPE = 0.2;
constexpr double AILUT_EPS = 1e-5;

template <typename Src> __device__ __forceinline__ float thumb_read(Src c);
template <> __device__ __forceinline__ float thumb_read<uint16_t>(uint16_t c) { return (float)c * (1.f / 65536.f); }      // (exact)
template <> __device__ __forceinline__ float thumb_read<uint8_t>(uint8_t c) { return (float)c / 255.f; }

// One thread = one thumbnail pixel, its three samples.  Source coordinates in integers, as ailut.axis: num = (2 j + 1) n - 256, a negative one 0; i0 = num >> 9,
// frac = (num & 511) / 512 (exact in fp32), i1 = min(i0 + 1, n - 1): i0 <= (511 n - 256) >> 9 < n.  a = fma(fx, v01 - v00, v00) and its twin, fma(fy, b - a, a):
// three roundings behind 16-bit samples, whose differences are exact.
template <typename Src>
__global__ __launch_bounds__(256) void to_float_thumb_kernel(const Src* __restrict__ src, float* __restrict__ dst, int H, int W, int rgb)
{
    const int oy = blockIdx.x, ox = threadIdx.x;          // (grid 256 x block 256: the thumbnail itself)
    long long ny = (2ll * oy + 1) * H - TS, nx = (2ll * ox + 1) * W - TS;
    if (ny < 0) ny = 0;
    if (nx < 0) nx = 0;
    const int y0 = (int)(ny >> 9), x0 = (int)(nx >> 9);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float fy = (float)(int)(ny & 511) * (1.f / 512.f), fx = (float)(int)(nx & 511) * (1.f / 512.f);
    const Src* const r0 = src + (long long)y0 * W * 3, * const r1 = src + (long long)y1 * W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = thumb_read<Src>(r0[3 * x0 + c]), v01 = thumb_read<Src>(r0[3 * x1 + c]), v10 = thumb_read<Src>(r1[3 * x0 + c]), v11 = thumb_read<Src>(r1[3 * x1 + c]);
        const float a = fmaf(fx, v01 - v00, v00), b = fmaf(fx, v11 - v10, v10);
        dst[(rgb ? c : 2 - c) * (TS * TS) + oy * TS + ox] = fmaf(fy, b - a, a);
    }
}

__device__ __forceinline__ double wave_sum(double v)          // a fixed butterfly: every lane ends with the same bits
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// CIN -> COUT channels, HIN x HIN -> HIN / 2 squared.  grid (pixel groups, COUT / CO_T), block 256 = 4 waves = (4 / KS pixel waves) x (KS input-channel slices).
// PG_IN: the pixel groups of the producer's partials (NORM_IN).  STATS: this block's output is normalised by its consumer.
template <int CIN, int COUT, int HIN, int CO_T, int KS, int PG_IN, bool NORM_IN, bool STATS>
__global__ __launch_bounds__(256) void to_output_ailut_conv_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                                                   const double* __restrict__ stat_in, const float* __restrict__ gamma, const float* __restrict__ beta, double* __restrict__ stat_out)
{
    constexpr int HO = HIN / 2, PIX = HO * HO, PW = 4 / KS, CK = CIN / KS;
    static_assert(PIX % (64 * PW) == 0 && CIN % KS == 0 && COUT % CO_T == 0, "whole waves, whole slices");
    __shared__ double s_mu[NORM_IN ? CIN : 1], s_sc[NORM_IN ? CIN : 1], s_be[NORM_IN ? CIN : 1];
    __shared__ double red[KS > 1 ? 4 * CO_T * 64 : 1];
    __shared__ double sred[STATS && PW > 1 ? PW * CO_T * 2 : 1];
    if constexpr (NORM_IN) {          // the producer's partials, channel by channel: TPC threads a channel, PER partials each in order, then a butterfly over the TPC
        constexpr int TPC = 256 / CIN, PER = PG_IN / TPC;
        static_assert(TPC >= 1 && TPC <= 64 && PG_IN % TPC == 0, "a channel's partials divide among its threads");
        const int c = threadIdx.x / TPC, sub = threadIdx.x % TPC;
        double s = 0., q = 0.;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const double* const p = stat_in + ((size_t)c * PG_IN + sub * PER + i) * 2;
            s += p[0];
            q += p[1];
        }
#pragma unroll
        for (int m = TPC / 2; m >= 1; m >>= 1) {
            s += __shfl_xor(s, m);
            q += __shfl_xor(q, m);
        }
        if (sub == 0) {
            const double mean = s * (1. / (HIN * HIN)), var = fmax(q * (1. / (HIN * HIN)) - mean * mean, 0.);          // (HIN^2 is a power of two: the products are exact divisions)
            s_mu[c] = mean;
            s_sc[c] = (double)gamma[c] / sqrt(var + AILUT_EPS);
            s_be[c] = (double)beta[c];
        }
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int pw = wave / KS, ks = wave % KS;
    const int p = (blockIdx.x * PW + pw) * 64 + lane;
    const int oy = p / HO, ox = p % HO, iy0 = 2 * oy - 1, ix0 = 2 * ox - 1;          // taps iy0 .. iy0 + 2 <= HIN - 1: only -1 is out of range
    const int co0 = blockIdx.y * CO_T;
    double acc[CO_T];
#pragma unroll
    for (int j = 0; j < CO_T; ++j) acc[j] = 0.;
    for (int c = ks * CK; c < (ks + 1) * CK; ++c) {
        const float* const pl = in + (size_t)c * (HIN * HIN);
        double v[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = iy0 + ky, ix = ix0 + kx;
                const bool ok = iy >= 0 && ix >= 0;
                double x = ok ? (double)pl[iy * HIN + ix] : 0.;
                if constexpr (NORM_IN) x = ok ? fma(x - s_mu[c], s_sc[c], s_be[c]) : 0.;
                v[3 * ky + kx] = x;
            }
        const float* const wc = w + ((size_t)co0 * CIN + c) * 9;          // (wave-uniform)
#pragma unroll
        for (int j = 0; j < CO_T; ++j)
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[j] = fma(v[k], (double)wc[(size_t)j * CIN * 9 + k], acc[j]);
    }
    if constexpr (KS > 1) {          // the slices meet: wave 0 of the pixel group adds them in slice order
#pragma unroll
        for (int j = 0; j < CO_T; ++j) red[(wave * CO_T + j) * 64 + lane] = acc[j];
        __syncthreads();
        if (ks == 0) {
#pragma unroll
            for (int j = 0; j < CO_T; ++j) {
                double a = red[((pw * KS) * CO_T + j) * 64 + lane];
#pragma unroll
                for (int k = 1; k < KS; ++k) a += red[((pw * KS + k) * CO_T + j) * 64 + lane];
                acc[j] = a;
            }
        }
    }
    double ds[CO_T], dq[CO_T];
    if (ks == 0) {
#pragma unroll
        for (int j = 0; j < CO_T; ++j) {
            const double z = acc[j] + (double)bias[co0 + j];
            const float y = (float)(z >= 0. ? z : z * AILUT_SLOPE);          // the layer's one rounding
            out[(size_t)(co0 + j) * PIX + p] = y;
            if constexpr (STATS) {
                ds[j] = wave_sum((double)y);
                dq[j] = wave_sum((double)y * (double)y);
            }
        }
    }
    if constexpr (STATS) {
        constexpr int PGROUPS = PIX / (64 * PW);
        if constexpr (PW == 1) {
            if (ks == 0 && lane == 0) {
#pragma unroll
                for (int j = 0; j < CO_T; ++j) {
                    double* const o = stat_out + ((size_t)(co0 + j) * PGROUPS + blockIdx.x) * 2;
                    o[0] = ds[j];
                    o[1] = dq[j];
                }
            }
        } else {          // the workgroup's pixel waves, in wave order
            if (ks == 0 && lane == 0) {
#pragma unroll
                for (int j = 0; j < CO_T; ++j) {
                    sred[(pw * CO_T + j) * 2] = ds[j];
                    sred[(pw * CO_T + j) * 2 + 1] = dq[j];
                }
            }
            __syncthreads();
            if (threadIdx.x < CO_T) {
                double s = sred[threadIdx.x * 2], q = sred[threadIdx.x * 2 + 1];
#pragma unroll
                for (int k = 1; k < PW; ++k) {
                    s += sred[(k * CO_T + threadIdx.x) * 2];
                    q += sred[(k * CO_T + threadIdx.x) * 2 + 1];
                }
                double* const o = stat_out + ((size_t)(co0 + threadIdx.x) * PGROUPS + blockIdx.x) * 2;
                o[0] = s;
                o[1] = q;
            }
        }
    }
}

// AdaptiveAvgPool2d(2) on the 128 x 8 x 8 map (every workgroup pools for itself: 32 KB from L2), then one wave per output of the two linear layers: lin[o] for
// o < ranks = W_h0 f + b_h0, behind them the 3 (d - 1) rows of W_g f + b_g.  A lane adds its eight products in order, a fixed butterfly adds the lanes.
__global__ __launch_bounds__(256) void to_output_ailut_heads_kernel(const float* __restrict__ act, const float* __restrict__ h0_w, const float* __restrict__ h0_b,
                                                                    const float* __restrict__ g_w, const float* __restrict__ g_b, float* __restrict__ lin, int ranks, int nout)
{
    __shared__ double feat[AILUT_FEATS];
    for (int f = threadIdx.x; f < AILUT_FEATS; f += 256) {          // feature c 4 + y 2 + x
        const float* const q = act + (f >> 2) * 64 + ((f >> 1) & 1) * 32 + (f & 1) * 4;
        double s = 0.;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += (double)q[i * 8 + j];
        feat[f] = s * 0.0625;
    }
    __syncthreads();
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= nout) return;
    const float* const row = o < ranks ? h0_w + (size_t)o * AILUT_FEATS : g_w + (size_t)(o - ranks) * AILUT_FEATS;
    double s = 0.;
#pragma unroll
    for (int i = 0; i < AILUT_FEATS / 64; ++i) s = fma((double)row[lane + 64 * i], feat[lane + 64 * i], s);
    s = wave_sum(s);
    if (lane == 0) lin[o] = (float)(s + (double)(o < ranks ? h0_b[o] : g_b[o - ranks]));
}

// table[i] = {sum_r bank[c d^3 + i][r] w[r]}, c = R, G, B, straight into the moe_lut3d handle's entries; the last workgroup's first three threads write a channel's
// vertices each: softmax over its d - 1 values and the cumulative sum as ONE sequential loop -- a sequential fp32 sum of non-negative terms cannot decrease, which
// is what lut3d.hip's search relies on and nothing else checks on the device.
__global__ __launch_bounds__(256) void to_output_ailut_table_kernel(const float* __restrict__ bank, const float* __restrict__ lin, float4* __restrict__ table, float* __restrict__ vert, int d, int ranks)
{
    const int n = d * d * d, i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        float y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* const row = bank + ((size_t)c * n + i) * ranks;
            double s = 0.;
            for (int r = 0; r < ranks; ++r) s = fma((double)row[r], (double)lin[r], s);
            y[c] = (float)s;
        }
        table[i] = make_float4(y[0], y[1], y[2], 0.f);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < 3) {
        const float* const z = lin + ranks + threadIdx.x * (d - 1);
        float* const v = vert + threadIdx.x * d;
        float top = z[0], sum = 0.f, at = 0.f;
        for (int j = 1; j < d - 1; ++j) top = fmaxf(top, z[j]);
        for (int j = 0; j < d - 1; ++j) sum += expf(z[j] - top);
        v[0] = 0.f;
        for (int j = 0; j < d - 1; ++j) {
            at += expf(z[j] - top) / sum;
            v[j + 1] = at;
        }
    }
}

template <int CIN, int COUT, int HIN, int CO_T, int KS, int PG_IN, bool NORM_IN, bool STATS>
void launch_conv(const AilutNet& n, int i, hipStream_t s)
{
    constexpr int PIX = (HIN / 2) * (HIN / 2), PGROUPS = PIX / (64 * (4 / KS));
    static_assert(!STATS || PGROUPS == AILUT_STAT_GROUPS[CIN == 3 ? 0 : CIN == 16 ? 1 : CIN == 32 ? 2 : 3], "the partials' layout is the consumer's");
    hipLaunchKernelGGL((to_output_ailut_conv_kernel<CIN, COUT, HIN, CO_T, KS, PG_IN, NORM_IN, STATS>), dim3(PGROUPS, COUT / CO_T), dim3(256), 0, s,
                       i ? n.act[i - 1] : n.thumb, n.w[i], n.b[i], n.act[i], i ? n.stat[i - 1] : nullptr, i ? n.gamma[i - 1] : nullptr, i ? n.beta[i - 1] : nullptr, STATS ? n.stat[i] : nullptr);
}

}  // namespace

// Checked by moe_ailut_run / moe_ailut_thumbnail: H, W of 1 at least with 3 H W within an int, src_bits in {8, 16}
void launch_ailut_thumb(const void* src, int src_bits, int H, int W, int rgb, float* dst, hipStream_t s)
{
    if (src_bits == 8) hipLaunchKernelGGL((to_float_thumb_kernel<uint8_t>), dim3(TS), dim3(TS), 0, s, (const uint8_t*)src, dst, H, W, rgb);
    else hipLaunchKernelGGL((to_float_thumb_kernel<uint16_t>), dim3(TS), dim3(TS), 0, s, (const uint16_t*)src, dst, H, W, rgb);
}

const char* launch_ailut_stage(const AilutNet& n, int stage, float4* table, float* vert, hipStream_t s)
{
    const int nout = n.ranks + 3 * (n.d - 1), points = n.d * n.d * n.d;
    switch (stage) {
    case 1: launch_conv<3, 16, 256, 4, 1, 1, false, true>(n, 0, s); break;
    case 2: launch_conv<16, 32, 128, 4, 2, AILUT_STAT_GROUPS[0], true, true>(n, 1, s); break;
    case 3: launch_conv<32, 64, 64, 4, 4, AILUT_STAT_GROUPS[1], true, true>(n, 2, s); break;
    case 4: launch_conv<64, 128, 32, 2, 4, AILUT_STAT_GROUPS[2], true, true>(n, 3, s); break;
    case 5: launch_conv<128, 128, 16, 1, 4, AILUT_STAT_GROUPS[3], true, false>(n, 4, s); break;
    case 6:
        hipLaunchKernelGGL(to_output_ailut_heads_kernel, dim3((nout + 3) / 4), dim3(256), 0, s, n.act[4], n.h0_w, n.h0_b, n.g_w, n.g_b, n.lin, n.ranks, nout);
        return "to_output_ailut_heads_kernel";
    default:
        hipLaunchKernelGGL(to_output_ailut_table_kernel, dim3((points + 255) / 256), dim3(256), 0, s, n.bank, n.lin, table, vert, n.d, n.ranks);
        return "to_output_ailut_table_kernel";
    }
    return "to_output_ailut_conv_kernel";
}
