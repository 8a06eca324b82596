// luma_args_check.cpp -- every refusal of moe_luma_split, moe_luma_merge, moe_stitch_luma and moe_run_plan_luma (include/moephoto_amd.h), called from a stand-alone
// program so that the argument validation in plan_run.cpp can run under the host sanitizers.  No device is touched: every call must return before its first HIP call.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       plan_run.cpp planner.cpp errors.cpp ../../tools/luma_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/luma_args_check
//   /tmp/luma_args_check          (exit status 0 and "luma_args_check: N refusals, all as declared")
//
// plan_run.cpp, planner.cpp and errors.cpp are compiled into the program with the sanitizers (the program's definitions win over the library's); the library only
// supplies the kernels' launchers those files refer to.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../include/moephoto_amd.h"

static int n_checked = 0, n_bad = 0;

static void expect(int rc, int want, const char* text, const char* what)
{
    ++n_checked;
    const char* msg = moe_last_error();
    if (rc != want || !msg || !strstr(msg, text)) {
        ++n_bad;
        fprintf(stderr, "%s: rc %d (want %d), message \"%s\" (want \"%s\" in it)\n", what, rc, want, msg ? msg : "(null)", text);
    }
}

int main()
{
    const int64_t grey[3] = {1, 100, 140}, two[3] = {2, 100, 140}, rgb[3] = {3, 100, 140};
    moe_plan *p1 = nullptr, *p2 = nullptr, *p3 = nullptr;
    if (moe_plan_create(grey, 1e12, 1e-3, 5, 2, 8, 48, &p1) || moe_plan_create(two, 1e12, 1e-3, 5, 2, 8, 48, &p2) || moe_plan_create(rgb, 1e12, 1e-3, 5, 2, 8, 48, &p3)) {
        fprintf(stderr, "moe_plan_create: %s\n", moe_last_error());
        return 2;
    }
    moe_net* net = nullptr;
    if (moe_net_create(MOE_ARCH_NET2X, 2, &net)) {
        fprintf(stderr, "moe_net_create: %s\n", moe_last_error());
        return 2;
    }
    alignas(16) float buf[16] = {0};
    const float* tiles = buf;
    void* dst = buf;
    void* odd = (char*)buf + 1;
    void* half = (char*)buf + 2;
    const int matrices[] = {-1, 3, 99}, orders[] = {-1, 2, 7}, planes[] = {-1, 0, 1, 2, 5}, bitses[] = {-8, 1, 10, 12, 32};
#define SP(img, dt, C, H, W, mat, ord, dy, dc) moe_luma_split(img, dt, C, 14000, 140, 1, H, W, mat, ord, dy, dc, 0, nullptr)
    expect(SP(nullptr, MOE_F32, 3, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "moe_luma_split: NULL", "split: img");
    expect(SP(buf, MOE_F32, 3, 2, 2, 0, 1, nullptr, dst), MOE_EINVAL, "NULL", "split: dst_y");
    expect(SP(buf, MOE_F32, 3, 2, 2, 0, 1, dst, nullptr), MOE_EINVAL, "NULL", "split: dst_c");
    for (int c : planes) expect(SP(buf, MOE_F32, c, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "planes (3, or 4", "split: planes");
    expect(SP(buf, MOE_U8, 3, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "dtype", "split: dtype u8");
    expect(SP(buf, MOE_U16, 3, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "dtype", "split: dtype u16");
    expect(SP(buf, 9, 3, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "dtype", "split: dtype 9");
    expect(SP(buf, MOE_F32, 3, 0, 2, 0, 1, dst, dst), MOE_EINVAL, "positive", "split: no rows");
    expect(SP(buf, MOE_F32, 3, 2, -1, 0, 1, dst, dst), MOE_EINVAL, "positive", "split: negative width");
    for (int m : matrices) expect(SP(buf, MOE_F32, 3, 2, 2, m, 1, dst, dst), MOE_EINVAL, "unknown matrix", "split: matrix");
    for (int o : orders) expect(SP(buf, MOE_F32, 3, 2, 2, 0, o, dst, dst), MOE_EINVAL, "unknown order", "split: order");
    expect(SP(odd, MOE_F16, 3, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "not aligned", "split: odd img");
    expect(SP(half, MOE_F32, 3, 2, 2, 0, 1, dst, dst), MOE_EINVAL, "not aligned", "split: img at 2 bytes for fp32");
    expect(SP(buf, MOE_F16, 3, 2, 2, 0, 1, odd, dst), MOE_EINVAL, "not aligned", "split: odd dst_y");
    expect(SP(buf, MOE_F16, 3, 2, 2, 0, 1, dst, half), MOE_EINVAL, "dst_c is not 4-byte aligned", "split: dst_c at 2 bytes");
#define MG(y, dt, c, C, H, W, mat, ord, bits, d, ddt) moe_luma_merge(y, dt, c, C, H, W, mat, ord, bits, d, ddt, 0, nullptr)
    expect(MG(nullptr, MOE_F32, buf, 3, 2, 2, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "moe_luma_merge: NULL", "merge: y");
    expect(MG(buf, MOE_F32, nullptr, 3, 2, 2, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "NULL", "merge: c");
    expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, 0, nullptr, MOE_F32), MOE_EINVAL, "NULL", "merge: dst");
    for (int c : planes) expect(MG(buf, MOE_F32, buf, c, 2, 2, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "colour planes (3, or 4", "merge: planes");
    expect(MG(buf, MOE_U16, buf, 3, 2, 2, 0, 1, 0, dst, MOE_U16), MOE_EINVAL, "canvas dtype", "merge: dtype");
    expect(MG(buf, MOE_F32, buf, 3, 0, 2, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "positive", "merge: size");
    for (int m : matrices) expect(MG(buf, MOE_F32, buf, 3, 2, 2, m, 1, 0, dst, MOE_F32), MOE_EINVAL, "unknown matrix", "merge: matrix");
    for (int o : orders) expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, o, 0, dst, MOE_F32), MOE_EINVAL, "unknown order", "merge: order");
    for (int b : bitses) expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, b, dst, MOE_U16), MOE_EINVAL, "bits (0 = the canvas, 8 or 16)", "merge: bits");
    expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, 0, dst, MOE_F16), MOE_EINVAL, "dst dtype must be the canvas dtype", "merge: canvas form in another dtype");
    expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, 8, dst, MOE_F32), MOE_EINVAL, "dst dtype must be MOE_U8 or MOE_U16", "merge: samples as floats");
    expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, 16, dst, MOE_U8), MOE_EINVAL, "16 bits do not fit MOE_U8", "merge: 16 bits in bytes");
    expect(MG(buf, MOE_F32, half, 3, 2, 2, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "c is not 4-byte aligned", "merge: c at 2 bytes");
    expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, 16, odd, MOE_U16), MOE_EINVAL, "dst is not aligned", "merge: odd dst at 16 bits");
    expect(MG(buf, MOE_F32, buf, 3, 2, 2, 0, 1, 0, half, MOE_F32), MOE_EINVAL, "dst is not aligned", "merge: fp32 dst at 2 bytes");
    expect(MG(odd, MOE_F16, buf, 3, 2, 2, 0, 1, 0, dst, MOE_F16), MOE_EINVAL, "y is not aligned", "merge: odd y");
#define ST(pl, t, P, cdt, c, mat, ord, bits, d, ddt) moe_stitch_luma(pl, 0, t, nullptr, P, cdt, c, mat, ord, bits, d, ddt, nullptr)
    expect(ST(nullptr, tiles, 1, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "moe_stitch_luma: NULL", "stitch: plan");
    expect(ST(p1, nullptr, 1, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "NULL", "stitch: tiles");
    expect(ST(p1, tiles, 1, MOE_F32, nullptr, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "NULL", "stitch: c");
    expect(ST(p1, tiles, 1, MOE_F32, buf, 0, 1, 0, nullptr, MOE_F32), MOE_EINVAL, "NULL", "stitch: dst");
    const int pools[] = {-1, 0, 3, 4};
    for (int P : pools) expect(ST(p1, tiles, P, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "pool planes (1", "stitch: pool planes");
    expect(ST(p1, tiles, 1, MOE_U8, buf, 0, 1, 0, dst, MOE_U8), MOE_EINVAL, "canvas dtype", "stitch: canvas dtype");
    for (int m : matrices) expect(ST(p1, tiles, 1, MOE_F16, buf, m, 1, 0, dst, MOE_F16), MOE_EINVAL, "unknown matrix", "stitch: matrix");
    for (int o : orders) expect(ST(p2, tiles, 2, MOE_F16, buf, 0, o, 0, dst, MOE_F16), MOE_EINVAL, "unknown order", "stitch: order");
    for (int b : bitses) expect(ST(p1, tiles, 1, MOE_F16, buf, 0, 0, b, dst, MOE_U16), MOE_EINVAL, "bits (0 = the canvas, 8 or 16)", "stitch: bits");
    expect(ST(p1, tiles, 1, MOE_F16, buf, 0, 0, 0, dst, MOE_F32), MOE_EINVAL, "dst dtype must be the canvas dtype", "stitch: canvas form in another dtype");
    expect(ST(p1, tiles, 1, MOE_F16, buf, 0, 0, 16, dst, MOE_U8), MOE_EINVAL, "16 bits do not fit MOE_U8", "stitch: 16 bits in bytes");
    expect(ST(p1, tiles, 1, MOE_F16, half, 0, 0, 16, dst, MOE_U16), MOE_EINVAL, "c is not 4-byte aligned", "stitch: c at 2 bytes");
    expect(ST(p1, tiles, 1, MOE_F16, buf, 0, 0, 16, odd, MOE_U16), MOE_EINVAL, "dst is not aligned", "stitch: odd dst");
    expect(ST(p1, (const float*)half, 1, MOE_F16, buf, 0, 0, 16, dst, MOE_U16), MOE_EINVAL, "tiles_dev is not 4-byte aligned", "stitch: pool at 2 bytes");
#define RP(n, pl, img, dt, c, mat, ord, bits, d, ddt) moe_run_plan_luma(n, pl, img, dt, 14000, 140, 1, c, mat, ord, bits, d, ddt, 0, nullptr)
    expect(RP(nullptr, p1, buf, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "moe_run_plan_luma: NULL", "run: net");
    expect(RP(net, nullptr, buf, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "NULL", "run: plan");
    expect(RP(net, p1, nullptr, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "NULL", "run: img");
    expect(RP(net, p1, buf, MOE_F32, nullptr, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "NULL", "run: c");
    expect(RP(net, p1, buf, MOE_F32, buf, 0, 1, 0, nullptr, MOE_F32), MOE_EINVAL, "NULL", "run: dst");
    expect(RP(net, p3, buf, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "the plan has 3 planes", "run: a three-plane plan");
    expect(RP(net, p1, buf, MOE_U16, buf, 0, 1, 0, dst, MOE_U16), MOE_EINVAL, "canvas dtype", "run: dtype");
    expect(RP(net, p1, buf, MOE_F32, buf, 5, 1, 0, dst, MOE_F32), MOE_EINVAL, "unknown matrix 5", "run: matrix");
    expect(RP(net, p2, buf, MOE_F32, buf, 0, 5, 0, dst, MOE_F32), MOE_EINVAL, "unknown order 5", "run: order");
    expect(RP(net, p1, buf, MOE_F32, buf, 0, 1, 12, dst, MOE_U16), MOE_EINVAL, "12 bits", "run: bits");
    expect(RP(net, p1, buf, MOE_F32, buf, 0, 1, 16, dst, MOE_U8), MOE_EINVAL, "do not fit", "run: 16 bits in bytes");
    expect(RP(net, p1, buf, MOE_F32, half, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "c is not 4-byte aligned", "run: c at 2 bytes");
    expect(RP(net, p1, buf, MOE_F32, buf, 0, 1, 16, odd, MOE_U16), MOE_EINVAL, "dst is not aligned", "run: odd dst");
    expect(RP(net, p1, half, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_EINVAL, "img_y is not aligned", "run: img at 2 bytes for fp32");
    expect(RP(net, p1, buf, MOE_F32, buf, 0, 1, 0, dst, MOE_F32), MOE_ESTATE, "moe_run_plan_luma: net is not finalized", "run: net state");
    expect(RP(net, p2, buf, MOE_F16, buf, 2, 0, 8, odd, MOE_U8), MOE_ESTATE, "net is not finalized", "run: an odd dst is fine at 8 bits");
    moe_net_destroy(net);
    moe_plan_destroy(p1);
    moe_plan_destroy(p2);
    moe_plan_destroy(p3);
    if (n_bad) {
        fprintf(stderr, "luma_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("luma_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
