// yuv_args_check.cpp -- every refusal of moe_stitch_yuv, moe_run_plan_yuv and moe_to_yuv (include/moephoto_amd.h), called from a stand-alone program so that the
// argument validation in plan_run.cpp can run under the host sanitizers.  No device is touched: every call must return before its first HIP call.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       plan_run.cpp planner.cpp errors.cpp ../../tools/yuv_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/yuv_args_check
//   /tmp/yuv_args_check          (exit status 0 and "yuv_args_check: N refusals, all as declared")
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
    const int64_t rgb[3] = {3, 100, 140}, grey[3] = {1, 100, 140}, rgba[3] = {4, 100, 140};
    moe_plan *p3 = nullptr, *p1 = nullptr, *p4 = nullptr;
    if (moe_plan_create(rgb, 1e12, 1e-3, 5, 2, 8, 48, &p3) || moe_plan_create(grey, 1e12, 1e-3, 5, 2, 8, 48, &p1) || moe_plan_create(rgba, 1e12, 1e-3, 5, 2, 8, 48, &p4)) {
        fprintf(stderr, "moe_plan_create: %s\n", moe_last_error());
        return 2;
    }
    moe_net* net = nullptr;
    if (moe_net_create(MOE_ARCH_NET2X, 2, &net)) {
        fprintf(stderr, "moe_net_create: %s\n", moe_last_error());
        return 2;
    }
    float buf[16] = {0};
    const float* tiles = buf;
    void* dst = buf;
#define SY(pl, t, cdt, depth, matrix, order, d) moe_stitch_yuv(pl, 0, t, nullptr, cdt, depth, matrix, order, d, nullptr)
    expect(SY(nullptr, tiles, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "moe_stitch_yuv: NULL", "stitch: plan");
    expect(SY(p3, nullptr, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "NULL", "stitch: tiles");
    expect(SY(p3, tiles, MOE_F32, 8, 0, 0, nullptr), MOE_EINVAL, "NULL", "stitch: dst");
    expect(SY(p1, tiles, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "1 planes (C must be 3)", "stitch: one plane");
    expect(SY(p4, tiles, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "4 planes (C must be 3)", "stitch: four planes");
    expect(SY(p3, tiles, MOE_U8, 8, 0, 0, dst), MOE_EINVAL, "canvas dtype", "stitch: canvas dtype");
    const int depths[] = {-8, 0, 7, 9, 11, 14, 17, 32};
    for (int d : depths) expect(SY(p3, tiles, MOE_F16, d, 0, 0, dst), MOE_EINVAL, "depth", "stitch: depth");
    expect(SY(p3, tiles, MOE_F16, 10, -1, 0, dst), MOE_EINVAL, "unknown matrix -1", "stitch: matrix");
    expect(SY(p3, tiles, MOE_F16, 10, 3, 0, dst), MOE_EINVAL, "unknown matrix 3", "stitch: matrix");
    expect(SY(p3, tiles, MOE_F16, 10, 1 << 30, 0, dst), MOE_EINVAL, "unknown matrix", "stitch: matrix");
    expect(SY(p3, tiles, MOE_F16, 10, 0, -1, dst), MOE_EINVAL, "unknown order -1", "stitch: order");
    expect(SY(p3, tiles, MOE_F16, 10, 0, 2, dst), MOE_EINVAL, "unknown order 2", "stitch: order");
#define RY(n, pl, img, cdt, depth, matrix, order, d) moe_run_plan_yuv(n, pl, img, MOE_F32, 14000, 140, 1, cdt, depth, matrix, order, d, 0, nullptr)
    expect(RY(nullptr, p3, buf, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "moe_run_plan_yuv: NULL", "run: net");
    expect(RY(net, nullptr, buf, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "NULL", "run: plan");
    expect(RY(net, p3, nullptr, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "NULL", "run: img");
    expect(RY(net, p3, buf, MOE_F32, 8, 0, 0, nullptr), MOE_EINVAL, "NULL", "run: dst");
    expect(RY(net, p1, buf, MOE_F32, 8, 0, 0, dst), MOE_EINVAL, "planes (C must be 3)", "run: one plane");
    expect(RY(net, p3, buf, MOE_U16, 8, 0, 0, dst), MOE_EINVAL, "canvas dtype", "run: canvas dtype");
    expect(RY(net, p3, buf, MOE_F32, 13, 0, 0, dst), MOE_EINVAL, "depth 13", "run: depth");
    expect(RY(net, p3, buf, MOE_F32, 16, 3, 0, dst), MOE_EINVAL, "unknown matrix 3", "run: matrix");
    expect(RY(net, p3, buf, MOE_F32, 16, 0, 2, dst), MOE_EINVAL, "unknown order 2", "run: order");
    expect(RY(net, p3, buf, MOE_F32, 16, 2, 1, dst), MOE_ESTATE, "moe_run_plan_yuv: net is not finalized", "run: net state");
#define TY(src, sdt, H, W, depth, matrix, order, d) moe_to_yuv(src, sdt, H, W, depth, matrix, order, d, 0, nullptr)
    expect(TY(nullptr, MOE_F32, 4, 4, 8, 0, 0, dst), MOE_EINVAL, "moe_to_yuv: NULL", "to: src");
    expect(TY(buf, MOE_F32, 4, 4, 8, 0, 0, nullptr), MOE_EINVAL, "NULL", "to: dst");
    expect(TY(buf, MOE_F32, 0, 4, 8, 0, 0, dst), MOE_EINVAL, "size", "to: H");
    expect(TY(buf, MOE_F32, 4, -1, 8, 0, 0, dst), MOE_EINVAL, "size", "to: W");
    expect(TY(buf, MOE_U16, 4, 4, 8, 0, 0, dst), MOE_EINVAL, "dtype", "to: dtype");
    expect(TY(buf, MOE_F32, 4, 4, 11, 0, 0, dst), MOE_EINVAL, "depth 11", "to: depth");
    expect(TY(buf, MOE_F32, 4, 4, 12, 7, 0, dst), MOE_EINVAL, "unknown matrix 7", "to: matrix");
    expect(TY(buf, MOE_F32, 4, 4, 12, 2, 5, dst), MOE_EINVAL, "unknown order 5", "to: order");
    moe_net_destroy(net);
    moe_plan_destroy(p3);
    moe_plan_destroy(p1);
    moe_plan_destroy(p4);
    if (n_bad) {
        fprintf(stderr, "yuv_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("yuv_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
