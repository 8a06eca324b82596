// planes_args_check.cpp -- every refusal of moe_planes_to_float, moe_stitch_planes and moe_run_plan_planes (include/moephoto_amd.h), called from a stand-alone program so
// that the argument validation in plan_run.cpp can run under the host sanitizers.  No device is touched: every call must return before its first HIP call.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       plan_run.cpp planner.cpp errors.cpp ../../tools/planes_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/planes_args_check
//   /tmp/planes_args_check          (exit status 0 and "planes_args_check: N refusals, all as declared")
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
    const int64_t grey[3] = {1, 100, 140}, chroma[3] = {2, 50, 70}, five[3] = {5, 100, 140};
    moe_plan *p1 = nullptr, *p2 = nullptr, *p5 = nullptr;
    if (moe_plan_create(grey, 1e12, 1e-3, 5, 2, 8, 48, &p1) || moe_plan_create(chroma, 1e12, 1e-3, 5, 2, 8, 48, &p2) || moe_plan_create(five, 1e12, 1e-3, 5, 2, 8, 48, &p5)) {
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
    void* two = (char*)buf + 2;
#define TF(src, depth, H, W, dy, dc, dt) moe_planes_to_float(src, depth, H, W, dy, dc, dt, 0, nullptr)
    expect(TF(nullptr, 8, 2, 2, dst, dst, MOE_F32), MOE_EINVAL, "moe_planes_to_float: NULL", "to_float: src");
    expect(TF(buf, 8, 2, 2, nullptr, dst, MOE_F32), MOE_EINVAL, "NULL", "to_float: dst_y");
    expect(TF(buf, 8, 2, 2, dst, nullptr, MOE_F32), MOE_EINVAL, "NULL", "to_float: dst_c");
    const int depths[] = {-8, 0, 7, 9, 11, 14, 17, 32};
    for (int d : depths) expect(TF(buf, d, 2, 2, dst, dst, MOE_F32), MOE_EINVAL, "depth", "to_float: depth");
    const int sizes[][2] = {{3, 2}, {2, 3}, {0, 2}, {2, 0}, {-2, 2}, {2, -2}, {1, 1}, {100, 141}, {101, 140}};
    for (auto& s : sizes) expect(TF(buf, 8, s[0], s[1], dst, dst, MOE_F32), MOE_EINVAL, "even", "to_float: size");
    expect(TF(buf, 8, 2, 2, dst, dst, MOE_U8), MOE_EINVAL, "dst dtype", "to_float: dst dtype u8");
    expect(TF(buf, 8, 2, 2, dst, dst, MOE_U16), MOE_EINVAL, "dst dtype", "to_float: dst dtype u16");
    expect(TF(buf, 8, 2, 2, dst, dst, 9), MOE_EINVAL, "dst dtype", "to_float: dst dtype 9");
    expect(TF(odd, 10, 2, 2, dst, dst, MOE_F32), MOE_EINVAL, "src is not 2-byte aligned", "to_float: odd src at 10 bits");
    expect(TF(odd, 16, 2, 2, dst, dst, MOE_F16), MOE_EINVAL, "src is not 2-byte aligned", "to_float: odd src at 16 bits");
    expect(TF(buf, 8, 2, 2, odd, dst, MOE_F16), MOE_EINVAL, "not aligned", "to_float: odd dst_y");
    expect(TF(buf, 8, 2, 2, dst, odd, MOE_F16), MOE_EINVAL, "not aligned", "to_float: odd dst_c");
    expect(TF(buf, 8, 2, 2, dst, two, MOE_F32), MOE_EINVAL, "not aligned", "to_float: dst_c at 2 bytes for fp32");
#define SP(pl, t, C, cdt, depth, d) moe_stitch_planes(pl, 0, t, nullptr, C, cdt, depth, d, nullptr)
    expect(SP(nullptr, tiles, 1, MOE_F32, 8, dst), MOE_EINVAL, "moe_stitch_planes: NULL", "stitch: plan");
    expect(SP(p1, nullptr, 1, MOE_F32, 8, dst), MOE_EINVAL, "NULL", "stitch: tiles");
    expect(SP(p1, tiles, 1, MOE_F32, 8, nullptr), MOE_EINVAL, "NULL", "stitch: dst");
    expect(SP(p1, tiles, 0, MOE_F32, 8, dst), MOE_EINVAL, "0 planes (1 to 4", "stitch: no plane");
    expect(SP(p1, tiles, -3, MOE_F32, 8, dst), MOE_EINVAL, "-3 planes (1 to 4", "stitch: negative planes");
    expect(SP(p1, tiles, 5, MOE_F32, 8, dst), MOE_EINVAL, "5 planes (1 to 4", "stitch: five planes");
    expect(SP(p2, tiles, 2, MOE_U8, 8, dst), MOE_EINVAL, "canvas dtype", "stitch: canvas dtype u8");
    expect(SP(p2, tiles, 2, MOE_U16, 8, dst), MOE_EINVAL, "canvas dtype", "stitch: canvas dtype u16");
    for (int d : depths) expect(SP(p2, tiles, 2, MOE_F16, d, dst), MOE_EINVAL, "depth", "stitch: depth");
    expect(SP(p2, tiles, 2, MOE_F16, 10, odd), MOE_EINVAL, "dst is not 2-byte aligned", "stitch: odd dst at 10 bits");
    expect(SP(p1, tiles, 1, MOE_F32, 16, odd), MOE_EINVAL, "dst is not 2-byte aligned", "stitch: odd dst at 16 bits");
#define RP(n, pl, img, cdt, depth, d) moe_run_plan_planes(n, pl, img, MOE_F32, 14000, 140, 1, cdt, depth, d, 0, nullptr)
    expect(RP(nullptr, p1, buf, MOE_F32, 8, dst), MOE_EINVAL, "moe_run_plan_planes: NULL", "run: net");
    expect(RP(net, nullptr, buf, MOE_F32, 8, dst), MOE_EINVAL, "NULL", "run: plan");
    expect(RP(net, p1, nullptr, MOE_F32, 8, dst), MOE_EINVAL, "NULL", "run: img");
    expect(RP(net, p1, buf, MOE_F32, 8, nullptr), MOE_EINVAL, "NULL", "run: dst");
    expect(RP(net, p5, buf, MOE_F32, 8, dst), MOE_EINVAL, "5 planes (1 to 4", "run: five planes");
    expect(RP(net, p1, buf, MOE_U16, 8, dst), MOE_EINVAL, "canvas dtype", "run: canvas dtype");
    expect(RP(net, p2, buf, MOE_F32, 13, dst), MOE_EINVAL, "depth 13", "run: depth");
    expect(RP(net, p2, buf, MOE_F16, 12, odd), MOE_EINVAL, "dst is not 2-byte aligned", "run: odd dst");
    expect(RP(net, p2, buf, MOE_F32, 16, dst), MOE_ESTATE, "moe_run_plan_planes: net is not finalized", "run: net state");
    expect(RP(net, p1, buf, MOE_F32, 8, odd), MOE_ESTATE, "net is not finalized", "run: an odd dst is fine at 8 bits");
    moe_net_destroy(net);
    moe_plan_destroy(p1);
    moe_plan_destroy(p2);
    moe_plan_destroy(p5);
    if (n_bad) {
        fprintf(stderr, "planes_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("planes_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
