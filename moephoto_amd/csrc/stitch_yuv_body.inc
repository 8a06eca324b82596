// The body of stitch_yuv_kernel and of its dithered twin stitch_yuv_dither_kernel (stitch.hip, which includes this text once in each): in scope are the kernel's
// parameters `a` (StitchArgs) and `y` (YuvEdge), its template parameters TD and R, `constexpr bool DITHER` and `const bool ordered`.  One text, because a kernel body
// that reaches its by-value arguments through a shared function is scheduled differently, and the undithered kernel keeps its code.
    static_assert(R % 2 == 0, "a thread owns whole row pairs");
    __shared__ int s_seam[256];
    __shared__ int s_nseam;
    if (threadIdx.x == 0) s_nseam = 0;
    __syncthreads();
    const int Y0 = blockIdx.y * R, X0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    const int cw = (a.out_w + 1) / 2, ch = (a.out_h + 1) / 2;
    TD* const py = (TD*)a.out;
    TD* const pu = py + (long long)a.out_h * a.out_w;
    TD* const pv = pu + (long long)ch * cw;
    const bool f16 = y.f16 != 0;
    if (X0 < a.out_w) {
        StitchCols k;
        if (!stitch_classify(a, X0, k)) s_seam[atomicAdd(&s_nseam, 1)] = threadIdx.x;
        else {
            StitchRun<TD, 8> oy[R];
            StitchRun<TD, 4> ou[R / 2], ov[R / 2];
            int sum[3][4];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const StitchFold<3> f = stitch_fold_row<3>(a, k, X0, min(Y0 + r, a.out_h - 1), 0, 3);
                int s[3][8];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[c][e] = yuv_sample16(f.v[c][e], f16);
#pragma unroll
                for (int e = 0; e < 8; ++e) oy[r].e[e] = (TD)yuv_luma(y, s[0][e], s[1][e], s[2][e], yuv_round<DITHER>(ordered, X0 + e, Y0 + r));      // (a replicated row is not stored)
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[c][e] = (r & 1 ? sum[c][e] : 0) + s[c][2 * e] + s[c][2 * e + 1];
                if (r & 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned rnd = yuv_round<DITHER>(ordered, X0 / 2 + e, (Y0 + r) / 2);
                        ou[r / 2].e[e] = (TD)yuv_chroma(y.ku, y, sum[0][e], sum[1][e], sum[2][e], rnd);
                        ov[r / 2].e[e] = (TD)yuv_chroma(y.kv, y, sum[0][e], sum[1][e], sum[2][e], rnd);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (Y0 + r >= a.out_h) break;
                stitch_store(py + (long long)(Y0 + r) * a.out_w + X0, oy[r]);
                if (!(r & 1)) {      // (the pair's second row may be the replicated one: the chroma row exists with the first)
                    const long long at = (long long)((Y0 + r) / 2) * cw + X0 / 2;
                    stitch_store(pu + at, ou[r / 2]);
                    stitch_store(pv + at, ov[r / 2]);
                }
            }
        }
    }
    __syncthreads();
    // The enlisted groups: 4 * (R / 2) blocks of 2 x 2 pixels each, 12 samples a block.  One thread folds ONE sample (as the other edges' seam pass does: a thread that
    // walked its block's twelve folds one after the other held the whole workgroup for twelve chains of dependent loads -- 216 us on the 8K canvas for the sample
    // edge's 203); the samples of 21 blocks meet in LDS and one thread per block converts and writes them.
    constexpr int PER = 4 * (R / 2), NB = 21;      // blocks of one group: (row pair, block), the block innermost;  blocks per pass: 21 * 12 = 252 threads
    __shared__ int s_smp[NB * 12];
    const int nblk = s_nseam * PER, t = threadIdx.x;
    auto origin = [&](int b, int& xa, int& ya) {
        const int gidx = b / PER, rem = b - gidx * PER;
        xa = (blockIdx.x * 256 + s_seam[gidx]) * 8 + (rem % 4) * 2; ya = Y0 + (rem / 4) * 2;
        return b < nblk && xa < a.out_w && ya < a.out_h;
    };
    for (int b0 = 0; b0 < nblk; b0 += NB) {          // (block-uniform)
        int xa, ya;
        if (t < NB * 12 && origin(b0 + t / 12, xa, ya)) {
            const int item = t % 12, c = item % 3, i = item / 6, j = (item / 3) & 1;          // sample (i, j, c) of the block: (row, column, plane), the plane innermost
            const int X = j ? min(xa + 1, a.out_w - 1) : xa, Y = i ? min(ya + 1, a.out_h - 1) : ya;      // (the odd last column / row: the edge pixel again)
            s_smp[t] = yuv_sample16(stitch_pixel(a, X, Y, c), f16);
        }
        __syncthreads();
        if (t < NB && origin(b0 + t, xa, ya)) {
            const int* q = s_smp + t * 12;
            int sum[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int* e = q + (i * 2 + j) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sum[c] += e[c];
                    if ((i && ya + 1 >= a.out_h) || (j && xa + 1 >= a.out_w)) continue;
                    py[(long long)(ya + i) * a.out_w + xa + j] = (TD)yuv_luma(y, e[0], e[1], e[2], yuv_round<DITHER>(ordered, xa + j, ya + i));
                }
            const long long at = (long long)(ya / 2) * cw + xa / 2;
            const unsigned rnd = yuv_round<DITHER>(ordered, xa / 2, ya / 2);
            pu[at] = (TD)yuv_chroma(y.ku, y, sum[0], sum[1], sum[2], rnd);
            pv[at] = (TD)yuv_chroma(y.kv, y, sum[0], sum[1], sum[2], rnd);
        }
        __syncthreads();
    }
