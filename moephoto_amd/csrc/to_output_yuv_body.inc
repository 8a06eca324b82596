// The body of to_output_yuv_kernel and of its dithered twin to_output_yuv_dither_kernel (stitch.hip, which includes this text once in each): in scope are the kernel's
// parameters src, dst, H, W and `y` (YuvEdge), its template parameters TS and TD, `constexpr bool DITHER` and `const bool ordered` (see stitch_yuv_body.inc).
    const int X0 = (blockIdx.x * 256 + threadIdx.x) * 8, ya = blockIdx.y * 2;
    if (X0 >= W) return;
    const int cw = (W + 1) / 2, ch = (H + 1) / 2;
    const long long HW = (long long)H * W;
    TD* const pu = dst + HW;
    TD* const pv = pu + (long long)ch * cw;
    const bool whole = X0 + 8 <= W;
    StitchRun<TD, 8> oy[2];
    int sum[3][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int Y = min(ya + i, H - 1);
        int s[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const TS* p = src + c * HW + (long long)Y * W;
            TS v[8];
            if (whole) stitch_mix_load8(p + X0, 1, ((uintptr_t)(p + X0) & 15) == 0, v);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = p[min(X0 + e, W - 1)];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s[c][e] = yuv_sample16((float)v[e], false);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[c][e] = (i ? sum[c][e] : 0) + s[c][2 * e] + s[c][2 * e + 1];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) oy[i].e[e] = (TD)yuv_luma(y, s[0][e], s[1][e], s[2][e], yuv_round<DITHER>(ordered, X0 + e, ya + i));
    }
    StitchRun<TD, 4> ou, ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned rnd = yuv_round<DITHER>(ordered, X0 / 2 + e, (int)blockIdx.y);
        ou.e[e] = (TD)yuv_chroma(y.ku, y, sum[0][e], sum[1][e], sum[2][e], rnd);
        ov.e[e] = (TD)yuv_chroma(y.kv, y, sum[0][e], sum[1][e], sum[2][e], rnd);
    }
    const long long at = (long long)blockIdx.y * cw + X0 / 2;
    if (whole) {
        stitch_store(dst + (long long)ya * W + X0, oy[0]);
        if (ya + 1 < H) stitch_store(dst + (long long)(ya + 1) * W + X0, oy[1]);
        stitch_store(pu + at, ou);
        stitch_store(pv + at, ov);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {      // (constant indices: a run indexed by a loop variable is moved to LDS)
            if (X0 + e >= W) break;
            dst[(long long)ya * W + X0 + e] = oy[0].e[e];
            if (ya + 1 < H) dst[(long long)(ya + 1) * W + X0 + e] = oy[1].e[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (X0 + 2 * e >= W) break;
            pu[at + e] = ou.e[e]; pv[at + e] = ov.e[e];
        }
    }
